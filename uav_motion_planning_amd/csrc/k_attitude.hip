// k_attitude.hip -- the kernels of qp_attitude.h as their own translation unit (kernel_instances.h: UAVQP_INSTANCES_ATTITUDE); no host code here.
#define UAVQP_KERNEL_TU
#include "qp_attitude.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_ATTITUDE

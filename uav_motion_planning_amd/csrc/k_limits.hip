// k_limits.hip -- the kernels of qp_limits.h as their own translation unit (kernel_instances.h: UAVQP_INSTANCES_LIMITS); no host code here.
#define UAVQP_KERNEL_TU
#include "qp_limits.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_LIMITS

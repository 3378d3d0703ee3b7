// k_moving.hip -- the kernels of qp_moving.h as their own translation unit (kernel_instances.h: UAVQP_INSTANCES_MOVING); no host code here.
#define UAVQP_KERNEL_TU
#include "qp_moving.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_MOVING

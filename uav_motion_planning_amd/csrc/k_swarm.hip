// k_swarm.hip -- the kernels of qp_swarm.h as their own translation unit (kernel_instances.h: UAVQP_INSTANCES_SWARM); no host code here.
#define UAVQP_KERNEL_TU
#include "qp_swarm.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_SWARM

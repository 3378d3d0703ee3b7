// k_swarm_opt.hip -- the kernels of qp_swarm_opt.h as their own translation unit (kernel_instances.h: UAVQP_INSTANCES_SWARM_OPT); no host code here.
#include "qp_esdf.h"   // (before UAVQP_KERNEL_TU, as in k_spacetime.hip: the plain kernels of the distance field are defined in k_esdf.hip alone)
#define UAVQP_KERNEL_TU
#include "qp_swarm_opt.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_SWARM_OPT

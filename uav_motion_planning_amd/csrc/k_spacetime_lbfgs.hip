// k_spacetime_lbfgs.hip -- the kernel of qp_spacetime_lbfgs.h as its own translation unit (kernel_instances.h: UAVQP_INSTANCES_SPACETIME_LBFGS); no host code here.
#include "qp_esdf.h"   // (before UAVQP_KERNEL_TU: the plain kernels of the distance field are defined in k_esdf.hip alone)
#define UAVQP_KERNEL_TU
#include "qp_spacetime_lbfgs.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_SPACETIME_LBFGS

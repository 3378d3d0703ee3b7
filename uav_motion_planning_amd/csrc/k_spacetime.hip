// k_spacetime.hip -- the kernels of qp_spacetime.h as their own translation unit (kernel_instances.h: UAVQP_INSTANCES_SPACETIME); no host code here.
#include "qp_esdf.h"   // (before UAVQP_KERNEL_TU: the plain kernels of the distance field are defined in k_esdf.hip alone; here only esdf_sample is used)
#define UAVQP_KERNEL_TU
#include "qp_spacetime.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_SPACETIME

// k_esdf.hip -- the kernels of qp_esdf.h as their own translation unit (kernel_instances.h: UAVQP_INSTANCES_ESDF); no host code here.
#define UAVQP_KERNEL_TU
#include "qp_esdf.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_ESDF

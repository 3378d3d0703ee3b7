// k_adjoint.hip -- the kernel of qp_adjoint.h as its own translation unit (kernel_instances.h: UAVQP_INSTANCES_ADJOINT); no host code here.
#define UAVQP_KERNEL_TU
#include "qp_adjoint.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_ADJOINT

// k_clearance_cert.hip -- the kernels of qp_clearance_cert.h as their own translation unit (kernel_instances.h: UAVQP_INSTANCES_CLEARANCE_CERT); no host code here.
#define UAVQP_KERNEL_TU
#include "qp_clearance_cert.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_CLEARANCE_CERT

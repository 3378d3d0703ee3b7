// k_separation_cert.hip -- the kernels of qp_separation_cert.h as their own translation unit (kernel_instances.h: UAVQP_INSTANCES_SEPARATION_CERT); no host code here.
#define UAVQP_KERNEL_TU
#include "qp_separation_cert.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_SEPARATION_CERT

// k_moving_cert.hip -- the kernels of qp_moving_cert.h as their own translation unit (kernel_instances.h: UAVQP_INSTANCES_MOVING_CERT); no host code here.
#define UAVQP_KERNEL_TU
#include "qp_moving_cert.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_MOVING_CERT

// k_envelope.hip -- the kernels of qp_envelope.h as their own translation unit (kernel_instances.h: UAVQP_INSTANCES_ENVELOPE); no host code here.
#define UAVQP_KERNEL_TU
#include "qp_envelope.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_ENVELOPE

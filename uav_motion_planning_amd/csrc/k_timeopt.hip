// k_timeopt.hip -- the kernels of qp_time_opt.h as their own translation unit (kernel_instances.h: UAVQP_INSTANCES_TIMEOPT); no host code here.
#define UAVQP_KERNEL_TU
#include "qp_time_opt.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_TIMEOPT

// k_wpopt.hip -- the kernels of qp_waypoint_opt.h as their own translation unit (kernel_instances.h: UAVQP_INSTANCES_WPOPT); no host code here.
#define UAVQP_KERNEL_TU
#include "qp_waypoint_opt.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_WPOPT

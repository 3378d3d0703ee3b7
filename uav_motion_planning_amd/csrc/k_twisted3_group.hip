// k_twisted3_group.hip -- solve_twisted_group_kernel<3, M, TILE, LPT> (qp_twisted.h): up to eight one-tile-per-wave solves of one shape in one launch.
#define UAVQP_KERNEL_TU
#include "qp_twisted.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_TWISTED3_GROUP

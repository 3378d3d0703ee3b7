// k_twisted3_group8.hip -- solve_twisted_group8_kernel<3, M> (qp_twisted.h): up to eight tile-4 solves of one shape in one launch, eight trajectories per wave.
#define UAVQP_KERNEL_TU
#include "qp_twisted.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_TWISTED3_GROUP8

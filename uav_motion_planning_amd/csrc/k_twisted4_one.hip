// k_twisted4_one.hip -- solve_twisted_kernel<4, M, TILE, LPT, true> (qp_twisted.h): the latency shapes for launches of one whole tile per wave.
#define UAVQP_KERNEL_TU
#include "qp_twisted.h"
#include "kernel_instances.h"
UAVQP_INSTANCES_TWISTED4_ONE

// What the host asks of csrc/kernel_instances.h without the HIP runtime: is there a group kernel for (r, M) at this tile, is there the
// group kernel with eight trajectories per wave?  Prints one line "r M group4 group8tile eight" for r = 3, 4 and M = 1 .. 24;
// tests/test_twisted_instances.py holds the lines against the lists it reads from the header's text.
#include <cstdio>

#include "kernel_instances.h"

int main() {
    for (int r = 3; r <= 4; ++r)
        for (int M = 1; M <= 24; ++M)
            std::printf("%d %d %d %d %d\n", r, M, (int)uavqp_twisted_group_exists(r, M, 4), (int)uavqp_twisted_group_exists(r, M, 8),
                        (int)uavqp_twisted_group8_exists(r, M));
    return 0;
}

// Host-only test of the slot carver (uav_motion_planning_amd/csrc/uavqp_ws.h): a wrong offset is a silent overlap of two kernels'
// state, so the layout rules are pinned here, without the HIP runtime.  Compiled and run by tests/test_ws_carve.py.
#include <cstdint>
#include <cstdio>

#include "uavqp_ws.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
            ++failures;                                                  \
        }                                                                \
    } while (0)

int main() {
    alignas(256) static char buffer[8192];
    const size_t sizes[] = {1, 256, 257, 0, 4000, 48, 0, 512};
    const int n_sizes = (int)(sizeof(sizes) / sizeof(sizes[0]));
    Carve c;
    int handle[16];
    size_t sum = 0;
    for (int k = 0; k < n_sizes; ++k) {
        handle[k] = c.add(sizes[k]);
        sum += align256(sizes[k]);
        const int gone = c.add(1000, false);   // an absent slot between every two present ones
        CHECK(gone == -1);
        CHECK(c.total == sum);                 // ... takes no room
    }
    CHECK(c.n == n_sizes && !c.overflow());
    CHECK(c.total == sum && sum <= sizeof(buffer));   // the total is the sum of the aligned sizes
    c.place(buffer);
    CHECK(c.at<char>(-1) == nullptr);
    CHECK(c.at<double>(-1) == nullptr);
    const char* end_of_previous = buffer;
    for (int k = 0; k < n_sizes; ++k) {
        CHECK(handle[k] == k);
        const char* p = c.at<char>(handle[k]);
        CHECK(p != nullptr);
        CHECK(((uintptr_t)p & 255u) == 0);     // every present slot starts on a 256-byte boundary
        CHECK(p >= end_of_previous);           // declaration order, no overlap
        CHECK(p == end_of_previous || k == 0 || (size_t)(p - end_of_previous) < 256);   // and no more than the padding between two slots
        end_of_previous = p + sizes[k];
    }
    CHECK(end_of_previous <= buffer + c.total);
    // a zero-sized slot takes no room and keeps its place: the next slot starts where it does
    CHECK(c.at<char>(handle[3]) == c.at<char>(handle[4]));
    // the same layout on another base (the mapped page behind its head): same offsets
    Carve d = c;
    d.place(buffer + 256);
    for (int k = 0; k < n_sizes; ++k) CHECK(d.at<char>(handle[k]) == c.at<char>(handle[k]) + 256);

    // capacity: exactly CAP declarations are fine, one more is refused -- remembered, and nothing written past the array
    struct Guarded {
        Carve c;
        unsigned long long canary = 0xC0FFEE1234567890ull;
    } g;
    for (int k = 0; k < Carve::CAP; ++k) CHECK(g.c.add(16) == k);
    CHECK(!g.c.overflow());
    const size_t full = g.c.total;
    CHECK(full == (size_t)Carve::CAP * 256);
    CHECK(g.c.add(16) == -1);
    CHECK(g.c.overflow());
    CHECK(g.c.add(16) == -1 && g.c.overflow());   // and stays refused
    CHECK(g.c.total == full);
    CHECK(g.canary == 0xC0FFEE1234567890ull);
    CHECK(Carve::CAP >= 34);                      // the corridor pipeline in rows mode

    if (failures == 0) std::printf("ws_carve OK\n");
    return failures == 0 ? 0 : 1;
}

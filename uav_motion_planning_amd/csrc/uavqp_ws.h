// uavqp_ws.h -- which bytes of which buffer belong to whom: the ONE offset accountant of the library (Carve) and the grow-only device
// buffers of a ctx (DevBuf; only where the including file has defined UAVQP_HIP -- the carver itself is plain size_t arithmetic and
// compiles without the HIP runtime: tests/cpp/test_ws_carve.cpp).  The staging of the host entries (uavqp_stage.h) sits on the same carver.
#pragma once
#include <cstddef>

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The sub-buffers of one call, laid out in the order they are declared; each starts on a 256-byte boundary (the specialised kernels are
// chosen only for 16-byte aligned arrays).  add() returns the slot's handle for at<T>(); a slot this call does not have (present = false)
// takes no room, its handle is -1 and at<T>(-1) is a null pointer.  A present slot of 0 bytes takes no room either and keeps its place.
// One declaration more than CAP is remembered (overflow()) and refuses the call where the layout is placed; nothing is written past the array.
struct Carve {
    static constexpr int CAP = 40;   // the largest site, the corridor pipeline in rows mode, declares 34
    size_t offset[CAP];
    int n = 0;
    size_t total = 0;       // sum of the aligned sizes = what the buffer is asked for
    char* base = nullptr;   // set by place() / carve_on(); the pointers are good for this call only (a later call may free the buffer)

    int add(size_t bytes, bool present = true) {
        if (!present) return -1;
        if (n >= CAP) return n = CAP + 1, -1;
        offset[n] = total;
        total += align256(bytes);
        return n++;
    }
    bool overflow() const { return n > CAP; }
    void place(void* at_base) { base = (char*)at_base; }   // (a bare pointer: the mapped page of the latency route behind MAPPED_HEAD)
    template <class T>
    T* at(int i) const { return i < 0 ? nullptr : (T*)(base + offset[i]); }
};

#ifdef UAVQP_HIP
// A device buffer the ctx owns and only ever grows.  dev_grow is the one place such a buffer is allocated: large enough -- nothing
// happens; otherwise the stream is synchronised (kernels of an earlier call may still use the old bytes), the buffer freed and exactly
// `bytes` allocated.  uavqp_destroy frees each with dev_free.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};
static int dev_grow(hipStream_t stream, DevBuf& b, size_t bytes) {
    if (bytes <= b.bytes) return UAVQP_OK;
    UAVQP_HIP(hipStreamSynchronize(stream));
    if (b.p) UAVQP_HIP(hipFree(b.p));
    b = DevBuf{};
    UAVQP_HIP(hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    return UAVQP_OK;
}
static void dev_free(DevBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b = DevBuf{};
}
// the layout `c` on buffer `b`, grown to c.total first
static int carve_on(hipStream_t stream, DevBuf& b, Carve& c) {
    if (c.overflow()) { g_last_error = "workspace layout: more slots than Carve::CAP"; return UAVQP_ERR_ALLOC; }
    const int rc = dev_grow(stream, b, c.total);
    if (rc == UAVQP_OK) c.place(b.p);
    return rc;
}
#endif

// Owners of HIP handles, shared by every host file of libtspgpu: device and
// pinned buffers, events, streams, and the pinned upload of a descriptor table.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cerrno>
#include <cstddef>

namespace tspgpu {

// HIP error -> the C ABI's errno-style code (tspgpu_strerror)
inline int hip_err(hipError_t e)
{
    if (e == hipSuccess) return 0;
    if (e == hipErrorOutOfMemory) return -ENOMEM;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return -ENODEV;
    return -EIO;
}

// Move-only owner of one HIP handle and its capacity (in the owner's unit: K2
// counts elements, the context counts bytes): a move leaves the source null
// with capacity 0, the destructor frees.  Frees need the owner's device
// current: tspgpu_search_destroy and the context's release set it first.
template <typename P, auto Free>
struct Owned {
    P p = nullptr;
    size_t cap = 0;
    Owned() = default;
    Owned(Owned &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) {
            reset();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~Owned() { reset(); }
    void reset()
    {
        if (p) (void)Free(p);
        p = nullptr, cap = 0;
    }
    operator P() const { return p; }
    P operator->() const { return p; }
};
template <typename T>
using DevBuf = Owned<T *, hipFree>;
template <typename T>
using Pinned = Owned<T *, hipHostFree>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;

// (re)allocate b for `count` elements
template <typename T>
hipError_t dev_alloc(DevBuf<T> &b, size_t count)
{
    b.reset();
    hipError_t e = hipMalloc((void **)&b.p, count * sizeof(T));
    if (e == hipSuccess) b.cap = count;
    return e;
}
template <typename T>
hipError_t pinned_alloc(Pinned<T> &b, size_t count)
{
    b.reset();
    hipError_t e = hipHostMalloc((void **)&b.p, count * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) b.cap = count;
    return e;
}

// Grow-only, capacity in BYTES: nothing when b holds `bytes` already;
// otherwise the old buffer is freed first (no copy) and at least 256 bytes are
// allocated.  On failure b is null with capacity 0 and the mapped error comes
// back (ensure_slots halves its chunk on -ENOMEM and calls again).
template <typename B, typename Alloc>
int reserve_bytes(B &b, size_t bytes, Alloc alloc)
{
    if (b.p && b.cap >= bytes) return 0;
    b.reset();
    const size_t n = bytes < 256 ? 256 : bytes;
    const hipError_t e = alloc((void **)&b.p, n);
    if (e != hipSuccess) {
        b.p = nullptr;
        return hip_err(e);
    }
    b.cap = n;
    return 0;
}
template <typename T>
int dev_reserve(DevBuf<T> &b, size_t bytes)
{
    return reserve_bytes(b, bytes, [](void **p, size_t n) { return hipMalloc(p, n); });
}
template <typename T>
int pinned_reserve(Pinned<T> &b, size_t bytes)
{
    return reserve_bytes(b, bytes, [](void **p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); });
}

// A table filled on the host and copied to the device from a pinned buffer,
// call after call: `read` fires when the copy has read the pinned buffer, and
// the next call waits for it before it writes there.
struct PinnedUpload {
    Pinned<void> host;
    DevBuf<void> dev;
    Event read;
    bool pending = false;
    // waits for the pending upload, grows both buffers -> *h, the pinned one
    int begin(size_t bytes, void **h)
    {
        hipError_t e = hipSuccess;
        if (pending) {
            if ((e = hipEventSynchronize(read)) != hipSuccess) return hip_err(e);
            pending = false;
        }
        int rc = dev_reserve(dev, bytes);
        if (!rc) rc = pinned_reserve(host, bytes);
        if (rc) return rc;
        if (!read && (e = hipEventCreateWithFlags(&read.p, hipEventDisableTiming)) != hipSuccess) return hip_err(e);
        *h = host.p;
        return 0;
    }
    // the copy of the first `bytes` on `stream`, and the event behind it
    int enqueue(size_t bytes, hipStream_t stream)
    {
        hipError_t e = hipMemcpyAsync(dev.p, host.p, bytes, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipEventRecord(read, stream);
        if (e != hipSuccess) return hip_err(e);
        pending = true;
        return 0;
    }
    // before the stream the upload may sit on is destroyed
    void drain()
    {
        if (pending) (void)hipEventSynchronize(read);
        pending = false;
    }
};

}  // namespace tspgpu

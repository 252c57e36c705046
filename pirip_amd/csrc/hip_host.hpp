// pirip_amd/csrc/hip_host.hpp -- what every handle of the library does with the HIP runtime on the host, defined once (library-private,
// HOST ONLY: the device headers fsk_device.hpp, demod_simd.hpp and ldpc_device.hpp do not include it). Everything here is static
// inline or hidden in a class: nothing is added to the library's dynamic symbols.
//
// Failure codes, one rule for every entry point: a failed device allocation is PIRIP_ERR_NOMEM, any other failure of a HIP call is
// PIRIP_ERR_HIP (a device that cannot be selected or made current is PIRIP_ERR_NO_DEVICE, as include/pirip_hip.h says).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <vector>

#include "../../include/pirip_hip.h"

#define PIRIP_HIPCHK(expr) do { if ((expr) != hipSuccess) return PIRIP_ERR_HIP; } while (0)
// (for calls that already answer with a PIRIP_* status: DevMem's, grow_dev)
#define PIRIP_TRY(expr) do { const int rc_ = (expr); if (rc_ != PIRIP_OK) return rc_; } while (0)

#pragma GCC visibility push(hidden)
namespace pirip {

// every entry point runs on the device its handle was created on, whatever the caller's current device is
static inline bool bind_device(int device)
{
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == device) return true;
    return hipSetDevice(device) == hipSuccess;
}

// create-time rule: device >= 0 must exist and becomes current, device < 0 takes the caller's current device; *chosen = the device now current
static inline int select_device(int device, int *chosen)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PIRIP_ERR_NO_DEVICE;
    if (device < 0) return hipGetDevice(chosen) == hipSuccess ? PIRIP_OK : PIRIP_ERR_NO_DEVICE;
    if (device >= ndev || !bind_device(device)) return PIRIP_ERR_NO_DEVICE;
    *chosen = device;
    return PIRIP_OK;
}

static inline int bytes_per_sample(int fmt)
{
    switch (fmt) {
    case PIRIP_IN_CU8_FSKDEMOD: case PIRIP_IN_CU8_CSDR: return 2;
    case PIRIP_IN_CS16: return 4;
    default: return 8;
    }
}

// Owner of a handle's device allocations, held by value in the handle. The handle keeps its typed pointers (they go into kernel
// arguments as they are); DevMem remembers every allocation made through it, so that nothing has to list them again to free them.
// The destructor frees what is left: `delete h` is the whole error path of a create function, and a destroy function is bind,
// synchronise, delete (destroy_handle).
class DevMem {
public:
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() { free_all(); }

    template <typename T>
    int alloc(T **p, size_t bytes)
    {
        void *q = nullptr;
        if (hipMalloc(&q, bytes) != hipSuccess) return PIRIP_ERR_NOMEM;
        if (q) owned_.push_back(Owned{q});
        *p = (T *)q;
        return PIRIP_OK;
    }
    // allocate and set every byte to `byte` (synchronous)
    template <typename T>
    int alloc_filled(T **p, int byte, size_t bytes)
    {
        PIRIP_TRY(alloc(p, bytes));
        if (bytes) PIRIP_HIPCHK(hipMemset(*p, byte, bytes));
        return PIRIP_OK;
    }
    // allocate and copy from the host (synchronous); an empty table still gets an allocation (16 bytes): its pointer goes to kernels
    template <typename T>
    int upload(T **p, const void *src, size_t bytes)
    {
        PIRIP_TRY(alloc(p, bytes ? bytes : 16));
        if (bytes) PIRIP_HIPCHK(hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice));
        return PIRIP_OK;
    }
    // free one allocation and null the handle's pointer to it (nullptr: nothing to do)
    template <typename T>
    void release(T **p)
    {
        if (!*p) return;
        for (Owned &o : owned_) if (o.p == (void *)*p) { o = owned_.back(); owned_.pop_back(); break; }
        (void)hipFree((void *)*p);
        *p = nullptr;
    }
    void free_all()
    {
        for (const Owned &o : owned_) (void)hipFree(o.p);
        owned_.clear();
    }

private:
    struct Owned { void *p; };          // (a hidden type of its own: the std::vector members instantiated for it stay out of the dynamic symbols)
    std::vector<Owned> owned_;
};

// Grow-on-demand device buffers to a capacity of `want`: wait for the work that may still use the old ones (GrowSync), free them, null
// them and the capacity, allocate anew (a buffer of 0 bytes is only freed), then record the capacity -- a failed allocation leaves the
// capacity at 0, so the next call starts again from nothing.
struct GrowBuf { void **p; size_t bytes; };
template <typename T> GrowBuf grow_buf(T **p, size_t bytes) { return GrowBuf{(void **)p, bytes}; }
enum class GrowSync { none, stream, device };
template <typename C>
int grow_dev(DevMem &mem, C *cap, C want, GrowSync sync, hipStream_t st, std::initializer_list<GrowBuf> bufs)
{
    if (sync == GrowSync::stream) PIRIP_HIPCHK(hipStreamSynchronize(st));
    if (sync == GrowSync::device) PIRIP_HIPCHK(hipDeviceSynchronize());
    for (const GrowBuf &b : bufs) mem.release(b.p);
    *cap = 0;
    for (const GrowBuf &b : bufs) if (b.bytes) PIRIP_TRY(mem.alloc(b.p, b.bytes));
    *cap = want;
    return PIRIP_OK;
}

// every destroy function: wait for the handle's work on its device, then free what it owns
template <class H>
static inline int destroy_handle(H *h, int device)
{
    if (!h) return PIRIP_ERR_BAD_ARG;
    (void)bind_device(device);
    (void)hipDeviceSynchronize();
    delete h;
    return PIRIP_OK;
}

// every counter getter: out.size() elements from the device, behind all the work enqueued on it
template <typename T>
static inline int read_back(int device, const T *d_src, std::vector<T> &out)
{
    if (!bind_device(device)) return PIRIP_ERR_NO_DEVICE;
    PIRIP_HIPCHK(hipDeviceSynchronize());
    PIRIP_HIPCHK(hipMemcpy(out.data(), d_src, sizeof(T) * out.size(), hipMemcpyDeviceToHost));
    return PIRIP_OK;
}

// Rows of IQ output, nsamp samples of bytes_per_sample each: pointer and stride are whole samples, and with more than one row the stride
// holds a row (rows would overlap). An entry point whose parent checked other things between the two asks twice: nrows = 1 asks the
// first only.
static inline int iq_rows_check(const void *d_out, size_t stride_bytes, int bytes_per_sample, int nrows, int64_t nsamp)
{
    if (((uintptr_t)d_out | stride_bytes) & (size_t)(bytes_per_sample - 1)) return PIRIP_ERR_BAD_ARG;
    if (nrows > 1 && stride_bytes < (size_t)nsamp * (size_t)bytes_per_sample) return PIRIP_ERR_BAD_ARG;
    return PIRIP_OK;
}

}  // namespace pirip
#pragma GCC visibility pop

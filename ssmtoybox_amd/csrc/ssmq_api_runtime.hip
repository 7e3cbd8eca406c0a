// C ABI of libssmq (include/ssmq.h), the runtime under every entry point: the thread-local error text, the per-thread contexts
// (stream + caches) with their pool, the handle guards, the environment-switch snapshot, and the device / memory / event / layout
// entry points.  No CPU fallback exists behind the library's entry points: every compute call ends in a HIP kernel launch or
// returns an error.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <string>
#include <unistd.h>
#include <unordered_map>
#include <vector>
#include "ssmq_host.h"

namespace ssmq {

static thread_local std::string g_err;

void set_error(const std::string &msg) { g_err = msg; }

int hip_fail(hipError_t e, const char *what) {
    if (e == hipSuccess) return SSMQ_OK;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return SSMQ_E_HIP;
}

// ---- per-thread contexts (ssmq_host.h) ------------------------------------------------------------------------------------
namespace {
struct CtxRegistry {
    std::mutex mu;                 // guards the free list, and every creation / destruction of a context's stream
    std::vector<Ctx *> free_list;
};
CtxRegistry &registry() {          // leaked on purpose: threads may end after the static destructors have run
    static CtxRegistry *r = new CtxRegistry;
    return *r;
}
std::atomic<unsigned> g_epoch_counter{0};
std::atomic<int> g_preferred_device{-1};     // the device of the last ssmq_set_device(): where a new thread starts
struct CtxHolder {
    Ctx *c = nullptr;
    ~CtxHolder() {                 // the thread ends: its context (stream, caches) goes back to the pool as it is
        if (!c) return;
        CtxRegistry &r = registry();
        std::lock_guard<std::mutex> l(r.mu);
        r.free_list.push_back(c);
        c = nullptr;
    }
};
thread_local CtxHolder t_holder;
thread_local bool t_first_call = true;
}  // namespace

// ---- switches: one snapshot of the environment, re-read only when the environment changed (ssmq_host.h) --------------------
namespace {
struct SwitchSnapshot {
    std::mutex mu;
    uint64_t sig = 0;
    std::unordered_map<std::string, const char *> vals;      // nullptr = unset
    std::deque<std::string> pool;                            // values are never freed: callers may hold the pointer
};
uint64_t environ_signature() {
    uint64_t h = 1469598103934665603ull;
    for (char **e = ::environ; e && *e; ++e) h = (h ^ (uint64_t)(uintptr_t)*e) * 1099511628211ull;
    return h ^ (uint64_t)(uintptr_t)::environ;
}
}  // namespace
const char *sw(const char *name) {
    static SwitchSnapshot c;
    std::lock_guard<std::mutex> g(c.mu);
    const uint64_t s = environ_signature();
    if (s != c.sig) {
        c.vals.clear();
        c.sig = s;
    }
    auto it = c.vals.find(name);
    if (it == c.vals.end()) {
        const char *v = getenv(name);
        if (v) {
            c.pool.emplace_back(v);
            v = c.pool.back().c_str();
        }
        it = c.vals.emplace(name, v).first;
    }
    return it->second;
}

Ctx &ctx() {
    if (!t_holder.c) {
        CtxRegistry &r = registry();
        std::lock_guard<std::mutex> l(r.mu);
        if (!r.free_list.empty()) {
            t_holder.c = r.free_list.back();
            r.free_list.pop_back();
        } else {
            t_holder.c = new Ctx;
        }
    }
    return *t_holder.c;
}

// Caches that hold memory / graphs of ONE device (the matrix-core scratch, the filter workspace with its captured launch
// loop, staging blocks): the calling thread's context drops them when it binds to another device, so that a workspace or graph
// of the previous device is never used from the new device's stream.
static void reset_device_caches() {
    drop_filter_cache();
    drop_theta_step_graphs();
    drop_gemm_scratch();
    drop_staging_arena();
    reset_wide_attributes();
    drop_multi_cache();
    drop_pipe_cache();
    Ctx &c = ctx();
    if (c.strip_buf) hipFree(c.strip_buf);
    c.strip_buf = nullptr;
    c.strip_bytes = 0;
}

int ensure_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no HIP device available (libssmq has no CPU fallback)");
        return SSMQ_E_HIP;
    }
    int dev = 0;
    SSMQ_HIP(hipGetDevice(&dev));
    if (t_first_call) {            // HIP's current device is per thread and starts at 0: a new thread starts where the library is
        t_first_call = false;
        const int pref = g_preferred_device.load();
        if (pref >= 0 && pref < n && pref != dev) {
            SSMQ_HIP(hipSetDevice(pref));
            dev = pref;
        }
    }
    Ctx &c = ctx();
    if (c.stream == nullptr || c.dev != dev) {
        std::lock_guard<std::mutex> l(registry().mu);
        if (c.stream != nullptr) {          // leaving a device: finish the context's work, release what it cached there
            hipSetDevice(c.dev);
            hipStreamSynchronize(c.stream);
            reset_device_caches();
            hipStreamDestroy(c.stream);
            c.stream = nullptr;
            SSMQ_HIP(hipSetDevice(dev));
        }
        SSMQ_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        c.dev = dev;
        c.epoch = ++g_epoch_counter;
    }
    return SSMQ_OK;
}

hipStream_t stream() { return ctx().stream; }
unsigned device_epoch() { return ctx().epoch; }

// A context that picks up handle `h` (locked by the caller) after another context used it: see HandleGuard.
static void adopt_handle(const ssmq_transform *h, Ctx &me) {
    if (!h || (h->owner == &me && h->owner_epoch == me.epoch)) return;
    if (h->owner) {
        // last used from another context: what that context queued on its stream - uploads of the handle's constants, buffers
        // built on first use, kernels still reading them - precedes whatever this context queues next.  Under the registry lock
        // only an EVENT is recorded on the owner's stream (the lock keeps the owner's stream alive); this context's stream
        // waits for it after the lock is released, so one thread's pending GPU work no longer stalls every other thread's
        // first call / hand-over behind the global mutex.  Everything the library does to a handle's device
        // blocks is stream-ordered (hipMemcpyAsync / kernels on the context's stream; hipFree synchronises the device).
        hipEvent_t ev = nullptr;
        {
            std::lock_guard<std::mutex> l(registry().mu);
            const Ctx *o = (const Ctx *)h->owner;
            if (o->stream && o->epoch == h->owner_epoch && hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
                if (o->dev != me.dev) hipSetDevice(o->dev);
                if (hipEventRecord(ev, o->stream) != hipSuccess) {
                    hipStreamSynchronize(o->stream);        // (cannot happen; the old behaviour as the fallback)
                    hipEventDestroy(ev);
                    ev = nullptr;
                }
                if (o->dev != me.dev) hipSetDevice(me.dev);
            }
        }
        if (ev) {
            if (me.stream == nullptr || hipStreamWaitEvent(me.stream, ev, 0) != hipSuccess) hipEventSynchronize(ev);
            hipEventDestroy(ev);         // (released once the event has completed)
        }
    }
    h->owner = &me;
    h->owner_epoch = me.epoch;
}

HandleGuard::HandleGuard(const ssmq_transform *h0, const ssmq_transform *h1) : a(h0), b(h1) {
    if (b == a) b = nullptr;
    if (!a) { a = b; b = nullptr; }
    if (a && b && b < a) std::swap(a, b);          // two handles: always in address order
    if (a) a->mu.lock();
    if (b) b->mu.lock();
    if (!a) return;
    (void)ensure_device();                         // (a failure is reported by the entry point's own call)
    Ctx &me = ctx();
    for (const ssmq_transform *h : {a, b}) adopt_handle(h, me);
}
MultiHandleGuard::MultiHandleGuard(std::vector<const ssmq_transform *> handles) : hs(std::move(handles)) {
    hs.erase(std::remove(hs.begin(), hs.end(), nullptr), hs.end());
    std::sort(hs.begin(), hs.end());
    hs.erase(std::unique(hs.begin(), hs.end()), hs.end());
    for (const ssmq_transform *h : hs) h->mu.lock();
    if (hs.empty()) return;
    (void)ensure_device();
    Ctx &me = ctx();
    for (const ssmq_transform *h : hs) adopt_handle(h, me);
}
MultiHandleGuard::~MultiHandleGuard() {
    for (auto it = hs.rbegin(); it != hs.rend(); ++it) (*it)->mu.unlock();
}
HandleGuard::~HandleGuard() {
    if (b) b->mu.unlock();
    if (a) a->mu.unlock();
}

// ---- layout conversion ---------------------------------------------------------------------------------------------
// AoS [B][n] <-> SoA [n][ld] through a padded LDS tile: both the global read and the global write are coalesced.
constexpr int kTile = 64;
__global__ __launch_bounds__(256) void k_aos_to_soa(const double *__restrict__ aos, double *__restrict__ soa, int n,
                                                     int64_t B, int64_t ld) {
    __shared__ double tile[kTile][kTile + 1];
    const int64_t b0 = (int64_t)blockIdx.x * kTile;
    const int e0 = blockIdx.y * kTile;
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;  // 64 x 4
    for (int r = ty; r < kTile; r += 4) {  // r: trajectory within tile, tx: element within tile
        const int64_t b = b0 + r;
        const int e = e0 + tx;
        if (b < B && e < n) tile[r][tx] = aos[b * n + e];
    }
    __syncthreads();
    for (int r = ty; r < kTile; r += 4) {  // r: element within tile, tx: trajectory
        const int64_t b = b0 + tx;
        const int e = e0 + r;
        if (b < B && e < n) soa[(int64_t)e * ld + b] = tile[tx][r];
    }
}
__global__ __launch_bounds__(256) void k_soa_to_aos(const double *__restrict__ soa, double *__restrict__ aos, int n,
                                                     int64_t B, int64_t ld) {
    __shared__ double tile[kTile][kTile + 1];
    const int64_t b0 = (int64_t)blockIdx.x * kTile;
    const int e0 = blockIdx.y * kTile;
    const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
    for (int r = ty; r < kTile; r += 4) {  // r: element, tx: trajectory
        const int64_t b = b0 + tx;
        const int e = e0 + r;
        if (b < B && e < n) tile[r][tx] = soa[(int64_t)e * ld + b];
    }
    __syncthreads();
    for (int r = ty; r < kTile; r += 4) {  // r: trajectory, tx: element
        const int64_t b = b0 + r;
        const int e = e0 + tx;
        if (b < B && e < n) aos[b * n + e] = tile[tx][r];
    }
}

__global__ void k_status_first(const int32_t *st, int64_t B, unsigned long long *first) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B && st[i] != 0) atomicMin(first, (unsigned long long)i);
}

}  // namespace ssmq

using namespace ssmq;

extern "C" {

int ssmq_version(void) { return SSMQ_VERSION; }
const char *ssmq_last_error(void) { return g_err.c_str(); }

int ssmq_device_count(int *n) {
    if (!n) return SSMQ_E_ARG;
    *n = 0;
    hipError_t e = hipGetDeviceCount(n);
    if (e != hipSuccess) {
        *n = 0;
        return hip_fail(e, "hipGetDeviceCount");
    }
    return SSMQ_OK;
}
int ssmq_set_device(int device) {
    SSMQ_HIP(hipSetDevice(device));
    t_first_call = false;
    g_preferred_device.store(device);            // threads that make their first call from now on start here
    return ensure_device();
}
int ssmq_current_device(void) {
    if (ensure_device()) return -1;
    return ctx().dev;
}
int ssmq_device_name(char *buf, int len) {
    if (!buf || len <= 0) return SSMQ_E_ARG;
    int rc = ensure_device();
    if (rc) return rc;
    int dev = 0;
    SSMQ_HIP(hipGetDevice(&dev));
    hipDeviceProp_t p;
    SSMQ_HIP(hipGetDeviceProperties(&p, dev));
    snprintf(buf, len, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
    return SSMQ_OK;
}
int ssmq_device_pci_bus_id(char *buf, int len) {
    if (!buf || len < 13) return SSMQ_E_ARG;
    int rc = ensure_device();
    if (rc) return rc;
    int dev = 0;
    SSMQ_HIP(hipGetDevice(&dev));
    SSMQ_HIP(hipDeviceGetPCIBusId(buf, len, dev));
    return SSMQ_OK;
}

int ssmq_malloc(void **dptr, size_t bytes) {
    if (!dptr) return SSMQ_E_ARG;
    int rc = ensure_device();
    if (rc) return rc;
    SSMQ_HIP(hipMalloc(dptr, bytes ? bytes : 8));
    return SSMQ_OK;
}
int ssmq_free(void *dptr) {
    if (!dptr) return SSMQ_OK;
    SSMQ_HIP(hipFree(dptr));
    return SSMQ_OK;
}
int ssmq_memcpy_h2d(void *dst, const void *src, size_t bytes) {
    int rc = ensure_device();
    if (rc) return rc;
    SSMQ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream()));
    SSMQ_HIP(hipStreamSynchronize(stream()));
    return SSMQ_OK;
}
int ssmq_memcpy_d2h(void *dst, const void *src, size_t bytes) {
    int rc = ensure_device();
    if (rc) return rc;
    SSMQ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream()));
    SSMQ_HIP(hipStreamSynchronize(stream()));
    return SSMQ_OK;
}
int ssmq_memcpy_d2d(void *dst, const void *src, size_t bytes) {
    int rc = ensure_device();
    if (rc) return rc;
    SSMQ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream()));
    return SSMQ_OK;
}
int ssmq_memset(void *dptr, int value, size_t bytes) {
    int rc = ensure_device();
    if (rc) return rc;
    SSMQ_HIP(hipMemsetAsync(dptr, value, bytes, stream()));
    return SSMQ_OK;
}
int ssmq_sync(void) {
    int rc = ensure_device();
    if (rc) return rc;
    SSMQ_HIP(hipStreamSynchronize(stream()));
    return SSMQ_OK;
}

int ssmq_aos_to_soa(const double *d_aos, double *d_soa, int n, int64_t B, int64_t ld) {
    if (!d_aos || !d_soa || n <= 0 || B < 0 || ld < B) return SSMQ_E_ARG;
    int rc = ensure_device();
    if (rc) return rc;
    if (B == 0) return SSMQ_OK;
    dim3 grid((unsigned)((B + kTile - 1) / kTile), (unsigned)((n + kTile - 1) / kTile));
    hipLaunchKernelGGL(k_aos_to_soa, grid, dim3(256), 0, stream(), d_aos, d_soa, n, B, ld);
    return hip_fail(hipGetLastError(), "k_aos_to_soa");
}
int ssmq_soa_to_aos(const double *d_soa, double *d_aos, int n, int64_t B, int64_t ld) {
    if (!d_aos || !d_soa || n <= 0 || B < 0 || ld < B) return SSMQ_E_ARG;
    int rc = ensure_device();
    if (rc) return rc;
    if (B == 0) return SSMQ_OK;
    dim3 grid((unsigned)((B + kTile - 1) / kTile), (unsigned)((n + kTile - 1) / kTile));
    hipLaunchKernelGGL(k_soa_to_aos, grid, dim3(256), 0, stream(), d_soa, d_aos, n, B, ld);
    return hip_fail(hipGetLastError(), "k_soa_to_aos");
}

int ssmq_event_create(void **ev) {
    if (!ev) return SSMQ_E_ARG;
    int rc = ensure_device();
    if (rc) return rc;
    hipEvent_t e;
    SSMQ_HIP(hipEventCreate(&e));
    *ev = (void *)e;
    return SSMQ_OK;
}
int ssmq_event_destroy(void *ev) {
    if (!ev) return SSMQ_OK;
    SSMQ_HIP(hipEventDestroy((hipEvent_t)ev));
    return SSMQ_OK;
}
int ssmq_event_record(void *ev) {
    if (!ev) return SSMQ_E_ARG;
    if (int rc = ensure_device()) return rc;        // a thread's FIRST call: its context has no stream yet (the NULL stream would not
                                                    // bracket the work the thread queues afterwards)
    SSMQ_HIP(hipEventRecord((hipEvent_t)ev, stream()));
    return SSMQ_OK;
}
int ssmq_event_elapsed_ms(void *start, void *stop, float *ms) {
    if (!start || !stop || !ms) return SSMQ_E_ARG;
    SSMQ_HIP(hipEventSynchronize((hipEvent_t)stop));
    SSMQ_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return SSMQ_OK;
}

int ssmq_status_first(const int32_t *d_status, int64_t B, int64_t *first) {
    if (!d_status || !first || B < 0) return SSMQ_E_ARG;
    int rc = ensure_device();
    if (rc) return rc;
    *first = -1;
    if (B == 0) return SSMQ_OK;
    unsigned long long *d_first = nullptr;
    SSMQ_HIP(hipMalloc((void **)&d_first, sizeof(unsigned long long)));
    unsigned long long init = ~0ull;
    SSMQ_HIP(hipMemcpyAsync(d_first, &init, sizeof(init), hipMemcpyHostToDevice, stream()));
    hipLaunchKernelGGL(k_status_first, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream(), d_status, B, d_first);
    unsigned long long res = ~0ull;
    hipError_t e = hipMemcpyAsync(&res, d_first, sizeof(res), hipMemcpyDeviceToHost, stream());
    if (e == hipSuccess) e = hipStreamSynchronize(stream());
    hipFree(d_first);
    if (e != hipSuccess) return hip_fail(e, "ssmq_status_first");
    *first = (res == ~0ull) ? -1 : (int64_t)res;
    return SSMQ_OK;
}

}  // extern "C"

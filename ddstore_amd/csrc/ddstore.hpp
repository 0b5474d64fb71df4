// ddstore_amd native store classes -- public C++ API.
//
// The reference exposes `class DDStore` as a C++ library (include/ddstore.hpp,
// used by test/demo.cxx); this header is the MI355X-native equivalent:
// `ddstore::DeviceStore` (HBM shards + hipIpc peers + CDNA4 gather kernels)
// and `ddstore::HostStore` (POSIX-shm CPU path), both usable from C++
// directly (see tools/demo_native.cpp) and bound to Python in
// ddstore_core.hip. Requires torch headers (tensors are the argument type).
#pragma once

#include <torch/extension.h>

#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>
#include <ATen/Parallel.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

#if defined(__x86_64__)
#include <emmintrin.h>  // SSE2 non-temporal stores (x86-64 baseline)
#endif

#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <limits>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "ddstore_kernels.h"

// roctx ranges so rocprofv3 --marker-trace attributes store phases
// (the reference has no tracing at all)
#include <roctracer/roctx.h>

namespace ddstore {

struct RoctxRange {
    explicit RoctxRange(const char* name) { roctxRangePushA(name); }
    ~RoctxRange() { roctxRangePop(); }
};

#define HIP_CHECK(expr)                                                        \
    do {                                                                       \
        hipError_t _e = (expr);                                                \
        TORCH_CHECK(_e == hipSuccess, "ddstore HIP error: ",                   \
                    hipGetErrorString(_e), " at " #expr);                      \
    } while (0)

inline int dds_type_of(at::ScalarType st) {
    switch (st) {
        case at::kByte: return DDS_U8;
        case at::kBool: return DDS_U8;  // stored/moved as u8 (0/1), NumPy layout
        case at::kInt: return DDS_I32;
        case at::kLong: return DDS_I64;
        case at::kFloat: return DDS_F32;
        case at::kDouble: return DDS_F64;
        case at::kHalf: return DDS_F16;
        case at::kBFloat16: return DDS_BF16;
        case at::kFloat8_e4m3fn: return DDS_F8E4M3;  // OCP fn, matches gfx950
        case at::kFloat8_e5m2: return DDS_F8E5M2;
        default:
            TORCH_CHECK(false, "ddstore: unsupported dtype ", st);
    }
}
inline int dds_type_of(const at::Tensor& t) { return dds_type_of(t.scalar_type()); }

inline std::vector<int64_t> make_prefix(const std::vector<int64_t>& counts) {
    std::vector<int64_t> prefix(counts.size() + 1, 0);
    for (size_t i = 0; i < counts.size(); ++i) prefix[i + 1] = prefix[i] + counts[i];
    return prefix;
}

// Parallel-for for the HostStore hot loops. at::parallel_for from an
// extension compiled without the wheel's OpenMP backend runs SEQUENTIALLY
// (measured: 9 GB/s vs torch index_select's 57 on identical shm data, r2).
// A spawn-per-call std::thread version fixed the 8-core container but
// collapsed on the 128-thread GPU-box host (127 thread spawns ~ the whole
// gather); this PERSISTENT pool parks at::get_num_threads()-1 workers on a
// condition variable and hands out ranges via an atomic cursor. Worker
// exceptions are rethrown in the caller (TORCH_CHECK-safe); the singleton
// is re-created after fork (pid check) and intentionally leaked.
class HostPool {
public:
    static HostPool& inst() {
        static std::mutex m;
        static HostPool* p = nullptr;
        static pid_t pid = 0;
        std::lock_guard<std::mutex> l(m);
        if (p == nullptr || pid != getpid()) {
            p = new HostPool();  // leaked: no teardown-order races at exit
            pid = getpid();
        }
        return *p;
    }

    void run(int64_t begin, int64_t end, int64_t step,
             const std::function<void(int64_t, int64_t)>& f) {
        // one task at a time: a second caller (e.g. another Python thread
        // gathering concurrently) must not overwrite the live task state
        std::lock_guard<std::mutex> excl(run_mx_);
        std::unique_lock<std::mutex> lk(m_);
        next_.store(begin, std::memory_order_relaxed);
        end_ = end;
        step_ = step;
        fn_ = &f;
        err_ = nullptr;
        active_ = (int)workers_.size();
        ++gen_;
        cv_work_.notify_all();
        lk.unlock();
        work();  // the caller participates
        lk.lock();
        cv_done_.wait(lk, [&] { return active_ == 0; });
        fn_ = nullptr;
        if (err_) std::rethrow_exception(err_);
    }

private:
    HostPool() {
        const int n = std::max(1, (int)at::get_num_threads()) - 1;
        workers_.reserve((size_t)n);
        for (int i = 0; i < n; ++i)
            workers_.emplace_back([this] { worker_loop(); });
    }

    void worker_loop() {
        uint64_t seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(m_);
            cv_work_.wait(lk, [&] { return gen_ != seen; });
            seen = gen_;
            lk.unlock();
            work();
            lk.lock();
            if (--active_ == 0) cv_done_.notify_all();
        }
    }

    void work() {
        try {
            for (;;) {
                const int64_t b = next_.fetch_add(step_);
                if (b >= end_) break;
                (*fn_)(b, std::min(b + step_, end_));
            }
        } catch (...) {
            std::lock_guard<std::mutex> l(em_);
            if (!err_) err_ = std::current_exception();
        }
    }

    std::mutex run_mx_, m_, em_;
    std::condition_variable cv_work_, cv_done_;
    std::vector<std::thread> workers_;
    std::atomic<int64_t> next_{0};
    int64_t end_ = 0, step_ = 1;
    const std::function<void(int64_t, int64_t)>* fn_ = nullptr;
    std::exception_ptr err_;
    uint64_t gen_ = 0;
    int active_ = 0;
};

template <typename F>
inline void host_parallel_for(int64_t begin, int64_t end, int64_t grain,
                              const F& f) {
    const int64_t n = end - begin;
    if (n <= 0) return;
    if (grain < 1) grain = 1;
    const int maxt = std::max(1, (int)at::get_num_threads());
    if (n <= grain || maxt <= 1) {
        f(begin, end);
        return;
    }
    const int64_t step = std::max<int64_t>(grain, n / (8 * maxt));
    std::function<void(int64_t, int64_t)> fn(std::cref(f));
    HostPool::inst().run(begin, end, step, fn);
}

// Row copy for the host gather path: the destination is written once and
// never re-read, so bypass the cache with SSE2 non-temporal stores where
// alignment allows (saves the read-for-ownership write traffic; measured
// against plain memcpy on the 8-core GPU-box host). Caller issues one
// _mm_sfence after the batch.
inline bool host_nt_enabled() {
    static const bool s = [] {
        const char* e = std::getenv("DDSTORE_HOST_NT");
        return e == nullptr || e[0] != '0';  // default on
    }();
    return s;
}

inline int host_prefetch_dist() {
    static const int s = [] {
        const char* e = std::getenv("DDSTORE_HOST_PF");
        return e ? atoi(e) : 8;
    }();
    return s;
}

inline void copy_row_nt(char* dst, const char* src, size_t nb) {
#if defined(__x86_64__)
    if (host_nt_enabled() && nb % 16 == 0 && ((uintptr_t)dst & 15) == 0) {
        for (size_t o = 0; o < nb; o += 16) {
            __m128i v = _mm_loadu_si128(reinterpret_cast<const __m128i*>(src + o));
            _mm_stream_si128(reinterpret_cast<__m128i*>(dst + o), v);
        }
        return;
    }
#endif
    std::memcpy(dst, src, nb);
}

inline void copy_rows_fence() {
#if defined(__x86_64__)
    _mm_sfence();
#endif
}

#ifndef MADV_COLLAPSE
#define MADV_COLLAPSE 25  // kernel >= 6.1; harmless EINVAL on older kernels
#endif

// Synchronously collapse a populated shm mapping to transparent huge pages
// (MADV_COLLAPSE works independent of the shmem THP policy, which boxes
// commonly leave at "never"): the random host gather is 4-KB-page TLB-bound
// on many-core hosts -- measured 251 GB/s vs 1.78 TB/s for the same gather
// from THP-backed malloc memory. Best-effort (errors ignored), one-time at
// registration; DDSTORE_HOST_THP=0 disables.
inline void try_collapse_hugepages(void* p, size_t bytes) {
    static const bool on = [] {
        const char* e = std::getenv("DDSTORE_HOST_THP");
        return e == nullptr || e[0] != '0';
    }();
    if (on && bytes >= (size_t)2 << 20) (void)madvise(p, bytes, MADV_COLLAPSE);
}

// Host-side owner lookup over the prefix directory (binary search; the
// reference's linear `sortedsearch` is src/ddstore.cxx:5-17).
inline int owner_of_host(const std::vector<int64_t>& prefix, int64_t row) {
    int lo = 0, hi = (int)prefix.size() - 2;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= row) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// DDSTORE_STRICT=1: out-of-range / over-capacity samples raise at the next
// host sync point (epoch_end) instead of being silently skipped+counted --
// the reference THROWS on a bad get (reference ddstore.hpp:210-214); the
// default here keeps the async hot path and counts (query()["oob_skipped"]).
inline bool strict_mode() {
    static const bool s = [] {
        const char* e = std::getenv("DDSTORE_STRICT");
        return e != nullptr && e[0] == '1';
    }();
    return s;
}

struct EpochFSM {
    bool fence_active = false;
    void begin() {
        TORCH_CHECK(!fence_active, "ddstore: epoch already began");  // ref ddstore.cxx:57
        fence_active = true;
    }
    void end() {
        TORCH_CHECK(fence_active, "ddstore: epoch has not begun");   // ref ddstore.cxx:71
        fence_active = false;
    }
};

// ===========================================================================
// What DeviceStore and HostStore share: the per-variable record and the
// checks that do not depend on where the shard lives
// ===========================================================================

// The CSR half of a registration.
struct CsrShape {
    int64_t nelems;                          // elements of the local shard
    const std::vector<int64_t>& nelems_all;  // per rank
    const at::Tensor& goff;                  // CPU int64 [nsamples_total + 1]
};

struct VarMeta {
    bool is_csr = false;
    int dds_t = 0;
    at::ScalarType st = at::kFloat;
    int64_t row_elems = 0;    // "disp" in reference terms
    int64_t itemsize = 0;
    int64_t nrows_local = 0;  // rows for fixed-stride; samples for CSR
    int64_t nelems_local = 0; // CSR: elements of the local shard
    std::vector<int64_t> prefix;
    std::vector<int64_t> elem_prefix;  // CSR
    void* base = nullptr;
    size_t base_bytes = 0;
    std::vector<void*> peers;
    // stats
    int64_t n_gather = 0, rows_gathered = 0, bytes_gathered = 0;

    // rows of the local shard's (n, row_elems) array
    int64_t local_count() const { return is_csr ? nelems_local : nrows_local; }
    size_t shard_bytes() const { return (size_t)(local_count() * row_elems * itemsize); }
    int64_t nrows_total() const { return prefix.back(); }
    // one gather call; `bytes` stays 0 where the device counts them
    // (DDS_CTR_ELEMS, see DeviceStore::query)
    void count(int64_t rows, int64_t bytes = 0) {
        n_gather += 1;
        rows_gathered += rows;
        bytes_gathered += bytes;
    }
};

// Everything a registration checks and records before it allocates, in the
// words of `op` ("add", "init", "add_csr", "init_csr"). `src` null = a shard
// zeroed now and filled later; `csr` null = fixed-stride, else `n_local` and
// `counts` are samples. `cpu_only`: the host store's sources live on the CPU.
inline void describe_var(VarMeta& v, const char* op, const at::Tensor* src,
                         at::ScalarType st, int64_t row_elems, int64_t n_local,
                         const std::vector<int64_t>& counts, const CsrShape* csr,
                         bool cpu_only) {
    if (src) {
        TORCH_CHECK(src->is_contiguous() && (!cpu_only || src->device().is_cpu()),
                    "ddstore ", op,
                    csr ? ": values must be contiguous" : ": array must be C-contiguous",
                    cpu_only ? " on CPU" : "");
        TORCH_CHECK(src->numel() == (csr ? csr->nelems : n_local) * row_elems,
                    "ddstore ", op, ": shape mismatch");
    }
    v.is_csr = csr != nullptr;
    v.st = st;
    v.dds_t = dds_type_of(st);
    v.itemsize = dds_itemsize(v.dds_t);
    v.row_elems = row_elems;  // CSR: feature width per element
    v.nrows_local = n_local;
    v.prefix = make_prefix(counts);
    if (csr) {
        v.nelems_local = csr->nelems;
        v.elem_prefix = make_prefix(csr->nelems_all);
        TORCH_CHECK(csr->goff.scalar_type() == at::kLong && csr->goff.is_contiguous() &&
                        csr->goff.device().is_cpu() &&
                        csr->goff.numel() == v.nrows_total() + 1,
                    "ddstore ", op, ": bad global offsets");
    }
}

// The checks of update (`elems` false: rows of a fixed-stride variable) and
// update_elems (true: elements of a CSR one; offsets are LOCAL, the Python
// layer translates a sample offset via the goff directory). Returns the byte
// offset of the fill in the local shard.
inline int64_t check_update(const VarMeta& v, bool elems, const at::Tensor& src,
                            int64_t offset, bool cpu_only) {
    if (elems) {
        TORCH_CHECK(v.is_csr, "ddstore update_elems: CSR variables only");
    } else {
        TORCH_CHECK(!v.is_csr, "ddstore update: not supported for CSR variables");
    }
    TORCH_CHECK(src.is_contiguous() && (!cpu_only || src.device().is_cpu()),
                "ddstore update: array must be C-contiguous", cpu_only ? " on CPU" : "");
    TORCH_CHECK(dds_itemsize(dds_type_of(src)) == v.itemsize,
                "ddstore update: itemsize mismatch");
    const int64_t n = src.numel() / std::max<int64_t>(v.row_elems, 1);
    TORCH_CHECK(src.numel() == n * v.row_elems, "ddstore update: shape mismatch");
    TORCH_CHECK(offset >= 0 && offset + n <= v.local_count(),
                "ddstore update: out of range");
    return offset * v.row_elems * v.itemsize;
}

// get_range, reference get semantics: dense [start, start+count) rows from
// ONE owner; throws if the range crosses a shard boundary
// (ddstore.hpp:197-248). The output checks, then (source, bytes) of the range
// in the owner's shard; the caller has checked that the peers are open.
inline void check_range_out(const VarMeta& v, const at::Tensor& out, int64_t count,
                            bool cpu_only) {
    TORCH_CHECK(!v.is_csr, "ddstore get: use get_csr for CSR variables");
    TORCH_CHECK(out.is_contiguous() && (!cpu_only || out.device().is_cpu()),
                "ddstore get: output must be C-contiguous", cpu_only ? " on CPU" : "");
    TORCH_CHECK(dds_itemsize(dds_type_of(out)) == v.itemsize,
                "ddstore get: itemsize mismatch");
    TORCH_CHECK(out.numel() == count * v.row_elems, "ddstore get: shape mismatch");
}
inline std::pair<const char*, size_t> owned_range(const VarMeta& v, int64_t start,
                                                  int64_t count) {
    TORCH_CHECK(start >= 0 && start < v.nrows_total(), "Invalid start on target");
    const int target = owner_of_host(v.prefix, start);
    TORCH_CHECK(start + count <= v.prefix[target + 1], "Invalid count on target");
    return {(const char*)v.peers[target] +
                (start - v.prefix[target]) * v.row_elems * v.itemsize,
            (size_t)count * v.row_elems * v.itemsize};
}

// The keys of query() both stores fill alike, in this order.
inline py::dict query_layout(const VarMeta& v) {
    py::dict d;
    d["nrows_local"] = v.nrows_local;
    d["nrows_total"] = v.nrows_total();
    d["disp"] = v.row_elems;
    d["itemsize"] = v.itemsize;
    d["is_csr"] = v.is_csr;
    d["prefix"] = v.prefix;
    if (v.is_csr) {
        d["nelems_local"] = v.nelems_local;
        d["elem_prefix"] = v.elem_prefix;
    }
    d["n_gather"] = v.n_gather;
    d["rows_gathered"] = v.rows_gathered;
    return d;
}

// Strict mode: raise if a variable has skipped samples (cumulative counters;
// reset via reset_counters after an intentional OOB probe).
inline void strict_check(const std::string& name, int64_t oob, int64_t cap) {
    TORCH_CHECK(oob == 0, "ddstore strict: variable '", name, "': ", oob,
                " out-of-range sample indices were skipped "
                "(DDSTORE_STRICT=1)");
    TORCH_CHECK(cap == 0, "ddstore strict: variable '", name, "': ", cap,
                " CSR samples skipped: output capacity buffer too "
                "small (DDSTORE_STRICT=1)");
}

// ===========================================================================
// DeviceStore
// ===========================================================================

struct DeviceVar : VarMeta {
    std::vector<char> opened;    // 1 where hipIpcOpenMemHandle was used
    void** d_peers = nullptr;
    int64_t* d_prefix = nullptr;
    unsigned long long* d_oob = nullptr;  // in-kernel OOB-index counter
    // CSR extras
    int64_t* d_elem_prefix = nullptr;
    int64_t* d_goff = nullptr;   // replicated global element offsets [ntotal+1]
};

class DeviceStore {
public:
    DeviceStore(int device, int rank, int nparts)
        : device_(device), rank_(rank), nparts_(nparts) {
        TORCH_CHECK(nparts >= 1 && nparts <= DDS_MAX_PARTS,
                    "ddstore: world size must be in [1, ", DDS_MAX_PARTS, "]");
        TORCH_CHECK(rank >= 0 && rank < nparts, "ddstore: bad rank");
    }
    ~DeviceStore() { free_all_noexcept(); }

    hipStream_t stream() const {
        return c10::hip::getCurrentHIPStream(device_).stream();
    }

    void add(const std::string& name, const at::Tensor& src, int64_t nrows,
             int64_t row_elems, std::vector<int64_t> nrows_all) {
        register_var(name, "add", &src, src.scalar_type(), row_elems, nrows, nrows_all,
                     nullptr);
    }

    void init(const std::string& name, int64_t nrows, int64_t row_elems,
              at::ScalarType st, std::vector<int64_t> nrows_all) {
        // reference: pre-allocate zeroed shard, fill later via update
        // (ddstore.hpp:110-179; README.md:107 -- no epoch required)
        register_var(name, "init", nullptr, st, row_elems, nrows, nrows_all, nullptr);
    }

    void add_csr(const std::string& name, const at::Tensor& values,
                 int64_t nsamples, int64_t nelems, int64_t row_elems,
                 std::vector<int64_t> nsamples_all, std::vector<int64_t> nelems_all,
                 const at::Tensor& goff_cpu) {
        // CSR first-class layout: the reference layers variable-length records
        // on an element-addressed store with disp=1 (HydraGNN
        // pattern); here offsets are replicated per GPU and the gather kernel
        // packs whole samples.
        const CsrShape csr{nelems, nelems_all, goff_cpu};
        register_var(name, "add_csr", &values, values.scalar_type(), row_elems, nsamples,
                     nsamples_all, &csr);
    }

    void init_csr(const std::string& name, int64_t nsamples, int64_t nelems,
                  int64_t row_elems, at::ScalarType st,
                  std::vector<int64_t> nsamples_all,
                  std::vector<int64_t> nelems_all, const at::Tensor& goff_cpu) {
        // CSR analog of init: lengths are fixed at registration (they define
        // the global offset directory), VALUES are zeroed and filled later
        // with update_elems -- the incremental-fill pattern the reference
        // supports for fixed-stride variables (ddstore.hpp:110-195,
        // README.md:107), extended to the first-class CSR layout.
        const CsrShape csr{nelems, nelems_all, goff_cpu};
        register_var(name, "init_csr", nullptr, st, row_elems, nsamples, nsamples_all,
                     &csr);
    }

    // purely local fills (reference ddstore.hpp:181-195), see check_update
    void update(const std::string& name, const at::Tensor& src, int64_t offset) {
        fill(name, src, offset, false);
    }
    void update_elems(const std::string& name, const at::Tensor& src,
                      int64_t elem_offset) {
        fill(name, src, elem_offset, true);
    }

    py::bytes ipc_handle(const std::string& name) {
        DeviceVar& v = var(name);
        hipIpcMemHandle_t h;
        HIP_CHECK(hipIpcGetMemHandle(&h, v.base));
        return py::bytes(reinterpret_cast<const char*>(&h), sizeof(h));
    }

    // Address of the local shard's allocation (an empty shard has one too):
    // what a same-process peer entry carries.
    uint64_t base_ptr(const std::string& name) {
        return (uint64_t)(uintptr_t)var(name).base;
    }

    // A same-process peer entry is exactly kLocalPeerBytes long: int64 pid,
    // uint64 device pointer, both in host byte order. It is valid only inside
    // the process that wrote it (a process cannot open an IPC handle it
    // created itself); any other pid raises. Returns the pointer.
    static constexpr size_t kLocalPeerBytes = 16;
    static_assert(sizeof(hipIpcMemHandle_t) != kLocalPeerBytes,
                  "a same-process peer entry must not be mistaken for an IPC handle");
    static uint64_t decode_local_peer(const std::string& entry) {
        TORCH_CHECK(entry.size() == kLocalPeerBytes,
                    "ddstore open_peers: a same-process peer entry has ",
                    kLocalPeerBytes, " bytes, got ", entry.size());
        int64_t pid = 0;
        uint64_t ptr = 0;
        std::memcpy(&pid, entry.data(), 8);
        std::memcpy(&ptr, entry.data() + 8, 8);
        TORCH_CHECK(pid == (int64_t)getpid(),
                    "ddstore open_peers: same-process peer entry written by pid ", pid,
                    ", this is pid ", (int64_t)getpid(),
                    " -- ranks in other processes must exchange IPC handles");
        TORCH_CHECK(ptr != 0, "ddstore open_peers: same-process peer entry without a pointer");
        return ptr;
    }

    // Finalize a variable: map peer shards (empty bytes => use own base) and
    // mirror the directory + pointer table to device memory. A peer's entry
    // is an IPC handle, or a same-process entry (decode_local_peer) whose
    // pointer is used as it is and never closed.
    // (reference analog: the MPI_Win_create collective, ddstore.hpp:56-62, or
    // the libfabric handshake's 3x Allgather, common.cxx:285-302)
    void open_peers(const std::string& name, const std::vector<std::string>& handles) {
        DeviceVar& v = var(name);
        TORCH_CHECK((int)handles.size() == nparts_, "ddstore open_peers: size mismatch");
        v.peers.assign(nparts_, nullptr);
        v.opened.assign(nparts_, 0);
        for (int r = 0; r < nparts_; ++r) {
            if (r == rank_) {
                v.peers[r] = v.base;
            } else if (handles[r].size() == kLocalPeerBytes) {
                v.peers[r] = (void*)(uintptr_t)decode_local_peer(handles[r]);
            } else {
                TORCH_CHECK(handles[r].size() == sizeof(hipIpcMemHandle_t),
                            "ddstore open_peers: bad handle bytes for rank ", r);
                hipIpcMemHandle_t h;
                std::memcpy(&h, handles[r].data(), sizeof(h));
                void* p = nullptr;
                hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
                TORCH_CHECK(e == hipSuccess,
                            "ddstore open_peers: hipIpcOpenMemHandle failed for peer rank ",
                            r, " (", hipGetErrorString(e),
                            ") -- peers must share one node/xGMI domain and "
                            "HSA_ENABLE_IPC_MODE_LEGACY=0 must be set");
                v.peers[r] = p;
                v.opened[r] = 1;
            }
        }
        // one device block: [peer ptrs | prefix | elem_prefix? | counters]
        size_t nb = nparts_ * sizeof(void*) + (nparts_ + 1) * 8 +
                    (v.is_csr ? (nparts_ + 1) * 8 : 0) + DDS_NCTR * 8;
        HIP_CHECK(hipMalloc((void**)&v.d_peers, nb));
        v.d_prefix = reinterpret_cast<int64_t*>(v.d_peers + nparts_);
        HIP_CHECK(hipMemcpy(v.d_peers, v.peers.data(), nparts_ * sizeof(void*),
                            hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(v.d_prefix, v.prefix.data(), (nparts_ + 1) * 8,
                            hipMemcpyHostToDevice));
        int64_t* tail = v.d_prefix + nparts_ + 1;
        if (v.is_csr) {
            v.d_elem_prefix = tail;
            HIP_CHECK(hipMemcpy(v.d_elem_prefix, v.elem_prefix.data(),
                                (nparts_ + 1) * 8, hipMemcpyHostToDevice));
            tail += nparts_ + 1;
        }
        v.d_oob = reinterpret_cast<unsigned long long*>(tail);
        HIP_CHECK(hipMemset(v.d_oob, 0, DDS_NCTR * 8));
    }

    void get_range(const std::string& name, int64_t start, int64_t count,
                   at::Tensor out) {
        DeviceVar& v = var(name);
        check_range_out(v, out, count, false);
        check_peers(v);
        const auto [src, nb] = owned_range(v, start, count);
        if (out.device().is_cpu()) {
            HIP_CHECK(hipStreamSynchronize(stream()));
            HIP_CHECK(hipMemcpy(out.data_ptr(), src, nb, hipMemcpyDeviceToHost));
        } else {
            TORCH_CHECK(out.device().index() == device_, "ddstore get: wrong device");
            HIP_CHECK(hipMemcpyAsync(out.data_ptr(), src, nb,
                                     hipMemcpyDeviceToDevice, stream()));
        }
        v.count(count, (int64_t)nb);
    }

    void gather(const std::string& name, const at::Tensor& idx, at::Tensor out) {
        // the batched hot path: one launch per minibatch
        RoctxRange rr_("ddstore::gather");
        gather_fixed(name, idx, out, Affine{});
    }

    void gather_affine(const std::string& name, const at::Tensor& idx,
                       at::Tensor out, double scale, double shift) {
        RoctxRange rr_("ddstore::gather_affine");
        gather_fixed(name, idx, out, Affine{true, (float)scale, (float)shift});
    }

    // gather_affine with one (scale, shift) pair per column.
    void gather_affine_cols(const std::string& name, const at::Tensor& idx,
                            at::Tensor out, const at::Tensor& scale,
                            const at::Tensor& shift) {
        RoctxRange rr_("ddstore::gather_affine_cols");
        gather_fixed(name, idx, out, Affine{true}, &scale, &shift);
    }

    // Column statistics of the local shard (fixed-stride: rows; CSR:
    // elements): a CPU f64 tensor (5, disp) = pivot, offset (mean = pivot +
    // offset), M2, min, max, as ddstore::column_stats writes it. Two kernels
    // on stream(), read back with one sync; scratch is
    // colstats_scratch_bytes, independent of the number of rows. Reads the
    // local shard only and touches no gather counter.
    at::Tensor column_stats(const std::string& name) {
        RoctxRange rr_("ddstore::column_stats");
        DeviceVar& v = var(name);
        const int64_t n = v.local_count();
        const int64_t d = v.row_elems;
        if (n == 0 || d == 0)
            return at::full({5, d}, std::numeric_limits<double>::quiet_NaN(),
                            at::TensorOptions().dtype(at::kDouble));
        auto opts = at::TensorOptions().dtype(at::kDouble).device(at::kCUDA, device_);
        at::Tensor out = at::empty({5, d}, opts);
        const size_t sb = ddstore::colstats_scratch_bytes(n, d, v.dds_t);
        at::Tensor scratch = at::empty({(int64_t)(sb / sizeof(double))}, opts);
        ddstore::column_stats(stream(), v.base, n, d, v.dds_t, scratch.data_ptr(),
                              out.data_ptr<double>());
        return out.cpu();
    }

    void gather_csr(const std::string& name, const at::Tensor& idx,
                    const at::Tensor& out_off, at::Tensor out, int64_t total_elems) {
        RoctxRange rr_("ddstore::gather_csr");
        DeviceVar& v = var(name);
        TORCH_CHECK(v.is_csr, "ddstore gather_csr: not a CSR variable");
        check_peers(v);
        check_idx(idx);
        check_idx(out_off);
        int64_t nidx = idx.numel();
        TORCH_CHECK(out_off.numel() == nidx + 1, "ddstore gather_csr: bad out_off");
        check_ragged_out(v, out);
        TORCH_CHECK(out.numel() >= total_elems * v.row_elems,
                    "ddstore gather_csr: output too small");
        // capacity passed to the kernel is the REAL buffer capacity: a sample
        // whose slice would end past it is skipped + counted, never written
        // out of bounds
        const int64_t cap = out.numel() / std::max<int64_t>(v.row_elems, 1);
        ddstore::gather_csr(stream(), csr_dir(v), idx.data_ptr<int64_t>(), nidx,
                            out_off.data_ptr<int64_t>(), v.row_elems * v.itemsize, cap,
                            out.data_ptr(), v.d_oob);
        v.count(nidx, total_elems * v.row_elems * v.itemsize);
    }

    // One-call CSR fetch: ONE fused kernel (per-sample lens + decoupled-
    // lookback exclusive scan + payload gather), no host round trips and no
    // intermediate lens/zeros launches. `out` is a capacity buffer
    // (>= worst-case batch elements); returns the [n+1] element-offset
    // tensor (device). True gathered-element stats accumulate in the
    // device counter block (the capacity would over-report).
    at::Tensor gather_csr_fast(const std::string& name, const at::Tensor& idx,
                               at::Tensor out) {
        RoctxRange rr_("ddstore::gather_csr_fast");
        DeviceVar& v = var(name);
        TORCH_CHECK(v.is_csr, "ddstore gather_csr: not a CSR variable");
        check_peers(v);
        check_idx(idx);
        return csr_fast(v, idx, out);
    }

    // Graph-batch fetch in one native call: the node variable exactly as
    // gather_csr_fast fetches it, then the edge-index variable's offsets
    // (csr_offsets), its edges relabelled to the packed batch
    // (gather_csr_relabel) and the batch vector plus both tails
    // (graph_fill); all on stream(), no host reads of device data. x_out's
    // capacity in elements is Ncap and batch_out holds exactly Ncap int64;
    // edge_out holds 2 * Ecap ids of the output dtype. Returns (ptr,
    // edge_ptr), both [n+1] and unclamped. Every element of batch_out and
    // edge_out is written.
    std::tuple<at::Tensor, at::Tensor> gather_graph(
        const std::string& node_name, const std::string& edge_name,
        const at::Tensor& idx, at::Tensor x_out, at::Tensor edge_out,
        at::Tensor batch_out, bool coo, int64_t edge_fill) {
        RoctxRange rr_("ddstore::gather_graph");
        DeviceVar& nv = var(node_name);
        DeviceVar& ev = var(edge_name);
        TORCH_CHECK(nv.is_csr && ev.is_csr, "ddstore gather_graph: not a CSR variable");
        check_peers(nv);
        check_peers(ev);
        check_idx(idx);
        TORCH_CHECK(ev.row_elems == 2 && (ev.dds_t == DDS_I32 || ev.dds_t == DDS_I64),
                    "ddstore gather_graph: the edge index must be an int32/int64 "
                    "variable with disp == 2");
        TORCH_CHECK(nv.prefix == ev.prefix,
                    "ddstore gather_graph: node and edge variables are sharded "
                    "differently");
        const int64_t nidx = idx.numel();
        const int64_t ncap = x_out.numel() / std::max<int64_t>(nv.row_elems, 1);
        TORCH_CHECK(batch_out.scalar_type() == at::kLong && batch_out.is_contiguous() &&
                        batch_out.device().is_cuda() &&
                        batch_out.device().index() == device_ &&
                        batch_out.numel() == ncap,
                    "ddstore gather_graph: batch_out must be a contiguous int64 "
                    "tensor of x_out's capacity on the store device");
        TORCH_CHECK(edge_out.is_contiguous() && edge_out.device().is_cuda() &&
                        edge_out.device().index() == device_ &&
                        edge_out.numel() % 2 == 0 &&
                        (edge_out.scalar_type() == at::kLong ||
                         (edge_out.scalar_type() == at::kInt && ev.dds_t == DDS_I32)),
                    "ddstore gather_graph: edge_out must be a contiguous int64 "
                    "tensor (int32 for an int32 variable) of 2 * Ecap elements "
                    "on the store device");
        const int out_t = dds_type_of(edge_out);
        TORCH_CHECK((uintptr_t)edge_out.data_ptr() % dds_itemsize(out_t) == 0 &&
                        (uintptr_t)batch_out.data_ptr() % 8 == 0,
                    "ddstore gather_graph: misaligned output");
        const int64_t ecap = edge_out.numel() / 2;
        TORCH_CHECK(out_t == DDS_I64 || ncap < (int64_t(1) << 31),
                    "ddstore gather_graph: int32 node ids need Ncap < 2^31");
        at::Tensor ptr = csr_fast(nv, idx, x_out);
        auto opts = at::TensorOptions().dtype(at::kLong).device(idx.device());
        at::Tensor edge_ptr = at::empty({nidx + 1}, opts);
        if (nidx == 0) {
            edge_ptr.zero_();
        } else {
            auto bopts = at::TensorOptions().dtype(at::kByte).device(idx.device());
            at::Tensor scratch = at::empty(
                {(int64_t)ddstore::csr_plan_scratch_bytes(nidx)}, bopts);
            const CsrDir edir = csr_dir(ev);
            ddstore::csr_offsets(stream(), edir, idx.data_ptr<int64_t>(), nidx,
                                 edge_ptr.data_ptr<int64_t>(), scratch.data_ptr(),
                                 ev.d_oob);
            ddstore::gather_csr_relabel(
                stream(), edir, idx.data_ptr<int64_t>(), nidx,
                ptr.data_ptr<int64_t>(), edge_ptr.data_ptr<int64_t>(), ncap, ecap,
                ev.dds_t, out_t, coo, edge_out.data_ptr(), ev.d_oob);
            ev.count(nidx);
        }
        ddstore::graph_fill(stream(), ptr.data_ptr<int64_t>(),
                            edge_ptr.data_ptr<int64_t>(), nidx, ncap, ecap, out_t,
                            coo, edge_fill, batch_out.data_ptr<int64_t>(),
                            edge_out.data_ptr());
        return {ptr, edge_ptr};
    }

    // Padded CSR fetch: one launch writes the dense (n, max_len, disp)
    // batch (cast / affine fused, pad broadcast from `pad_bits`, the raw
    // bits of one output element) and the true per-sample lengths. The
    // output shape does not depend on the data: no plan, no scratch, no
    // capacity semantics. True gathered-element stats accumulate in the
    // device counter block, as for gather_csr_fast.
    void gather_csr_padded(const std::string& name, const at::Tensor& idx,
                           at::Tensor out, at::Tensor lengths, int64_t max_len,
                           int64_t pad_bits, bool affine, double scale,
                           double shift) {
        RoctxRange rr_("ddstore::gather_csr_padded");
        padded(name, idx, out, lengths, max_len, pad_bits,
               Affine{affine, (float)scale, (float)shift});
    }

    // gather_csr_padded with one (scale, shift) pair per column of an element.
    void gather_csr_padded_cols(const std::string& name, const at::Tensor& idx,
                                at::Tensor out, at::Tensor lengths, int64_t max_len,
                                int64_t pad_bits, const at::Tensor& scale,
                                const at::Tensor& shift) {
        RoctxRange rr_("ddstore::gather_csr_padded_cols");
        padded(name, idx, out, lengths, max_len, pad_bits, Affine{true}, &scale, &shift);
    }

    void csr_lens(const std::string& name, const at::Tensor& idx, at::Tensor lens) {
        DeviceVar& v = var(name);
        TORCH_CHECK(v.is_csr, "ddstore csr_lens: not a CSR variable");
        check_peers(v);
        check_idx(idx);
        TORCH_CHECK(lens.scalar_type() == at::kLong && lens.is_contiguous() &&
                        lens.device().is_cuda() && lens.numel() == idx.numel(),
                    "ddstore csr_lens: bad lens tensor");
        // the lengths only: a bad index gets 0 here and is counted once, by
        // the gather_csr that follows (counting here too doubled oob_skipped)
        ddstore::csr_lens(stream(), csr_dir(v), idx.data_ptr<int64_t>(), idx.numel(),
                          lens.data_ptr<int64_t>(), nullptr, nullptr);
    }

    void scatter_local(const std::string& name, const at::Tensor& local_idx,
                       const at::Tensor& src) {
        // reshuffle placement: src row r -> local row local_idx[r]
        DeviceVar& v = var(name);
        TORCH_CHECK(!v.is_csr, "ddstore scatter_local: CSR not supported");
        check_idx(local_idx);
        TORCH_CHECK(src.is_contiguous() && src.device().is_cuda() &&
                        dds_type_of(src) == v.dds_t,
                    "ddstore scatter_local: bad src");
        TORCH_CHECK(src.numel() == local_idx.numel() * v.row_elems,
                    "ddstore scatter_local: shape mismatch");
        check_peers(v);  // d_oob lives in the metadata block
        ddstore::scatter_rows_local(stream(), v.base, v.nrows_local, v.row_elems,
                                    v.dds_t, local_idx.data_ptr<int64_t>(),
                                    local_idx.numel(), src.data_ptr(), v.d_oob);
    }

    // Zero-copy view of the local shard as a torch tensor (does NOT own).
    at::Tensor local_shard(const std::string& name) {
        DeviceVar& v = var(name);
        auto opts = at::TensorOptions().dtype(v.st).device(at::kCUDA, device_);
        return at::from_blob(v.base, {v.local_count(), v.row_elems}, opts);
    }

    void epoch_begin() {
        fsm_.begin();
        HIP_CHECK(hipStreamSynchronize(stream()));
    }
    void epoch_end() {
        fsm_.end();
        HIP_CHECK(hipStreamSynchronize(stream()));
        if (strict_mode()) check_strict();
    }
    bool epoch_active() const { return fsm_.fence_active; }

    void check_strict() {
        for (auto& kv : vars_) {
            DeviceVar& v = kv.second;
            if (!v.d_oob) continue;
            unsigned long long ctrs[DDS_NCTR] = {0, 0, 0};
            HIP_CHECK(hipMemcpy(ctrs, v.d_oob, DDS_NCTR * 8,
                                hipMemcpyDeviceToHost));
            strict_check(kv.first, (int64_t)ctrs[DDS_CTR_OOB], (int64_t)ctrs[DDS_CTR_CAP]);
        }
    }

    py::dict query(const std::string& name) {
        DeviceVar& v = var(name);
        py::dict d = query_layout(v);
        int64_t bytes = v.bytes_gathered;
        if (v.d_oob) {
            unsigned long long ctrs[DDS_NCTR] = {0, 0, 0};
            HIP_CHECK(hipStreamSynchronize(stream()));
            HIP_CHECK(hipMemcpy(ctrs, v.d_oob, DDS_NCTR * 8,
                                hipMemcpyDeviceToHost));
            d["oob_skipped"] = (int64_t)ctrs[DDS_CTR_OOB];
            d["cap_skipped"] = (int64_t)ctrs[DDS_CTR_CAP];
            // gather_csr_fast accounts true elements device-side (the
            // capacity-buffer size would over-report)
            bytes += (int64_t)ctrs[DDS_CTR_ELEMS] * v.row_elems * v.itemsize;
        }
        d["bytes_gathered"] = bytes;
        return d;
    }

    // Zero a variable's skip/stat counters (after an intentional OOB test,
    // or between bench phases).
    void reset_counters(const std::string& name) {
        DeviceVar& v = var(name);
        if (v.d_oob) {
            HIP_CHECK(hipStreamSynchronize(stream()));
            HIP_CHECK(hipMemset(v.d_oob, 0, DDS_NCTR * 8));
        }
        v.n_gather = v.rows_gathered = v.bytes_gathered = 0;
    }

    bool has(const std::string& name) const { return vars_.count(name) > 0; }

    void free_var(const std::string& name) {
        auto it = vars_.find(name);
        TORCH_CHECK(it != vars_.end(), "ddstore: unknown variable '", name, "'");
        release(it->second);
        vars_.erase(it);
    }

    void free_all() {
        for (auto& kv : vars_) release(kv.second);
        vars_.clear();
    }

private:
    void free_all_noexcept() noexcept {
        try { free_all(); } catch (...) { /* after runtime teardown */ }
    }

    void check_new(const std::string& name) {
        TORCH_CHECK(!vars_.count(name), "ddstore: variable '", name, "' already exists");
    }
    DeviceVar& var(const std::string& name) {
        auto it = vars_.find(name);
        TORCH_CHECK(it != vars_.end(), "ddstore: unknown variable '", name, "'");
        return it->second;
    }
    void check_peers(const DeviceVar& v) {
        TORCH_CHECK(v.d_peers != nullptr,
                    "ddstore: variable not finalized (open_peers not called)");
    }
    void check_idx(const at::Tensor& idx) {
        TORCH_CHECK(idx.scalar_type() == at::kLong && idx.is_contiguous() &&
                        idx.device().is_cuda() && idx.device().index() == device_,
                    "ddstore: indices must be a contiguous int64 tensor on the store device");
    }

    void alloc_base(DeviceVar& v, size_t bytes) {
        hipError_t e = hipSetDevice(device_);
        TORCH_CHECK(e == hipSuccess, "ddstore: hipSetDevice failed");
        v.base_bytes = bytes < 256 ? 256 : bytes;
        HIP_CHECK(hipMalloc(&v.base, v.base_bytes));
    }

    void ingest(void* dst_base, const at::Tensor& src, int64_t byte_off) {
        char* dst = (char*)dst_base + byte_off;
        size_t nb = (size_t)src.numel() * src.element_size();
        if (nb == 0) return;
        if (src.device().is_cpu()) {
            HIP_CHECK(hipMemcpy(dst, src.data_ptr(), nb, hipMemcpyHostToDevice));
        } else {
            TORCH_CHECK(src.device().index() == device_, "ddstore: wrong source device");
            HIP_CHECK(hipMemcpyAsync(dst, src.data_ptr(), nb,
                                     hipMemcpyDeviceToDevice, stream()));
            HIP_CHECK(hipStreamSynchronize(stream()));
        }
    }

    void release(DeviceVar& v) {
        if (!v.base) return;
        for (int r = 0; r < (int)v.peers.size(); ++r)
            if (v.opened.size() > (size_t)r && v.opened[r] && v.peers[r])
                (void)hipIpcCloseMemHandle(v.peers[r]);
        v.peers.clear();
        if (v.d_peers) (void)hipFree(v.d_peers);
        if (v.d_goff) (void)hipFree(v.d_goff);
        (void)hipFree(v.base);
        v.base = nullptr;
        v.d_peers = nullptr;
        v.d_goff = nullptr;
    }

    // The one registration body (arguments as describe_var): allocate, fill
    // from `src` or with zeros, upload the CSR offsets, release on any throw.
    void register_var(const std::string& name, const char* op, const at::Tensor* src,
                      at::ScalarType st, int64_t row_elems, int64_t n_local,
                      const std::vector<int64_t>& counts, const CsrShape* csr) {
        check_new(name);
        DeviceVar v;
        describe_var(v, op, src, st, row_elems, n_local, counts, csr, false);
        alloc_base(v, v.shard_bytes());
        try {
            if (src) {
                ingest(v.base, *src, 0);
            } else {
                HIP_CHECK(hipMemsetAsync(v.base, 0, v.base_bytes, stream()));
                HIP_CHECK(hipStreamSynchronize(stream()));
            }
            if (csr) {
                size_t gbytes = (size_t)csr->goff.numel() * 8;
                HIP_CHECK(hipMalloc((void**)&v.d_goff, gbytes));
                HIP_CHECK(hipMemcpy(v.d_goff, csr->goff.data_ptr<int64_t>(), gbytes,
                                    hipMemcpyHostToDevice));
            }
        } catch (...) {
            release(v);
            throw;
        }
        vars_[name] = std::move(v);
    }

    // body of update and update_elems
    void fill(const std::string& name, const at::Tensor& src, int64_t offset, bool elems) {
        DeviceVar& v = var(name);
        ingest(v.base, src, check_update(v, elems, src, offset, false));
    }

    // The only places that spell a variable's directory for the launchers
    // (void** converts to const void* const* without a cast).
    RowDir row_dir(const DeviceVar& v) const {
        return {v.d_peers, v.d_prefix, v.peers.data(), v.prefix.data(), nparts_};
    }
    CsrDir csr_dir(const DeviceVar& v) const {
        return {v.d_peers, v.d_prefix, v.d_elem_prefix, nparts_, v.d_goff,
                v.nrows_total()};
    }

    // The output check of a gather, in the caller's words: contiguous and on
    // the store device.
    void check_out(const at::Tensor& out, const char* msg) const {
        TORCH_CHECK(out.is_contiguous() && out.device().is_cuda() &&
                        out.device().index() == device_, msg);
    }
    // The ragged CSR forms ask for any GPU and the store dtype instead.
    static void check_ragged_out(const DeviceVar& v, const at::Tensor& out) {
        TORCH_CHECK(out.is_contiguous() && out.device().is_cuda() &&
                        dds_type_of(out) == v.dds_t,
                    "ddstore gather_csr: bad output tensor");
    }

    // One per-column affine vector: `n` contiguous floats on the store
    // device, 16-B aligned (the kernels load them as vectors).
    const float* affine_vec(const at::Tensor& t, int64_t n) const {
        TORCH_CHECK(t.scalar_type() == at::kFloat && t.is_contiguous() &&
                        t.device().is_cuda() && t.device().index() == device_ &&
                        t.numel() == n,
                    "ddstore: a per-column affine vector must be a contiguous float32 "
                    "tensor of disp = ", n, " values on the store device");
        TORCH_CHECK(((uintptr_t)t.data_ptr()) % 16 == 0,
                    "ddstore: a per-column affine vector must be 16-byte aligned");
        return t.data_ptr<float>();
    }
    static bool float_out(int out_t) {
        return out_t == DDS_F32 || out_t == DDS_F16 || out_t == DDS_BF16;
    }

    // The fixed-stride gather body: gather (xf off), gather_affine (the
    // scalar pair in xf) and gather_affine_cols (`scale` / `shift` given: one
    // pair per column, which also limits the row width).
    void gather_fixed(const std::string& name, const at::Tensor& idx, at::Tensor& out,
                      Affine xf, const at::Tensor* scale = nullptr,
                      const at::Tensor* shift = nullptr) {
        DeviceVar& v = var(name);
        TORCH_CHECK(!v.is_csr, "ddstore gather: use gather_csr for CSR variables");
        check_peers(v);
        check_idx(idx);
        const int64_t nidx = idx.numel();
        check_out(out, "ddstore gather: output must be a contiguous tensor on the store "
                       "device");
        TORCH_CHECK(out.numel() == nidx * v.row_elems, "ddstore gather: shape mismatch");
        // byte move only for the SAME dds type (bool aliases u8); any other
        // dtype pair converts numerically -- a same-size pair like f16->bf16
        // must NOT silently reinterpret bits (the CPU path converts too)
        const int out_t = dds_type_of(out);
        TORCH_CHECK(!xf.on || float_out(out_t),
                    "ddstore gather: affine output must be f32/f16/bf16");
        if (scale) {
            TORCH_CHECK(v.row_elems < (int64_t(1) << 31), "ddstore gather: row too long");
            xf.d_scale = affine_vec(*scale, v.row_elems);
            xf.d_shift = affine_vec(*shift, v.row_elems);
        }
        ddstore::gather_rows(stream(), row_dir(v), idx.data_ptr<int64_t>(), nidx,
                             v.row_elems, v.dds_t, out_t, xf, out.data_ptr(), v.d_oob);
        v.count(nidx, nidx * v.row_elems * v.itemsize);
    }

    // The padded CSR gather body, `xf`, `scale` and `shift` as for
    // gather_fixed. Bytes are counted on the device (DDS_CTR_ELEMS, see query).
    void padded(const std::string& name, const at::Tensor& idx, at::Tensor& out,
                at::Tensor& lengths, int64_t max_len, int64_t pad_bits, Affine xf,
                const at::Tensor* scale = nullptr, const at::Tensor* shift = nullptr) {
        DeviceVar& v = var(name);
        TORCH_CHECK(v.is_csr, "ddstore gather_csr_padded: not a CSR variable");
        check_peers(v);
        check_idx(idx);
        const int64_t nidx = idx.numel();
        TORCH_CHECK(max_len >= 1, "ddstore gather_csr_padded: max_len must be >= 1");
        check_out(out, "ddstore gather_csr_padded: output must be a contiguous tensor "
                       "on the store device");
        TORCH_CHECK(out.numel() == nidx * max_len * v.row_elems,
                    "ddstore gather_csr_padded: shape mismatch");
        TORCH_CHECK(lengths.scalar_type() == at::kLong && lengths.is_contiguous() &&
                        lengths.device().is_cuda() &&
                        lengths.device().index() == device_ &&
                        lengths.numel() == nidx,
                    "ddstore gather_csr_padded: bad lengths tensor");
        const int out_t = dds_type_of(out);
        TORCH_CHECK(!xf.on || float_out(out_t),
                    "ddstore gather_csr_padded: affine output must be f32/f16/bf16");
        if (scale) {
            TORCH_CHECK(v.row_elems >= 1 && v.row_elems < (int64_t(1) << 31) / 16,
                        "ddstore gather_csr_padded: bad element width for a column affine");
            xf.d_scale = affine_vec(*scale, v.row_elems);
            xf.d_shift = affine_vec(*shift, v.row_elems);
        }
        ddstore::gather_csr_padded(
            stream(), csr_dir(v), idx.data_ptr<int64_t>(), nidx, v.row_elems, max_len,
            v.dds_t, out_t, xf, (uint64_t)pad_bits, out.data_ptr(),
            lengths.data_ptr<int64_t>(), v.d_oob);
        v.count(nidx);
    }

    // body of gather_csr_fast, shared with gather_graph; `v` and `idx` are
    // checked by the caller. Bytes are counted on the device, as in `padded`.
    at::Tensor csr_fast(DeviceVar& v, const at::Tensor& idx, at::Tensor out) {
        const int64_t nidx = idx.numel();
        check_ragged_out(v, out);
        auto opts = at::TensorOptions().dtype(at::kLong).device(idx.device());
        at::Tensor off = at::empty({nidx + 1}, opts);
        if (nidx == 0) {
            off.zero_();
            return off;
        }
        const int64_t cap = out.numel() / std::max<int64_t>(v.row_elems, 1);
        const int64_t elem_bytes = v.row_elems * v.itemsize;
        auto bopts = at::TensorOptions().dtype(at::kByte).device(idx.device());
        at::Tensor scratch = at::empty(
            {(int64_t)ddstore::csr_plan_scratch_bytes(nidx)}, bopts);
        const int64_t desc_cap =
            cap / ddstore::csr_item_elems(elem_bytes) + nidx;
        // 2 i64 per item; uninitialised on purpose: the gather only acts on
        // slots the plan wrote in this call (see gather_csr_balanced)
        at::Tensor desc = at::empty({2 * desc_cap}, opts);
        ddstore::gather_csr_balanced(
            stream(), csr_dir(v), idx.data_ptr<int64_t>(), nidx, elem_bytes, cap,
            off.data_ptr<int64_t>(), out.data_ptr(), v.d_oob,
            scratch.data_ptr(), desc.data_ptr<int64_t>(), desc_cap);
        v.count(nidx);
        return off;
    }

    int device_;
    int rank_;
    int nparts_;
    EpochFSM fsm_;
    std::map<std::string, DeviceVar> vars_;
};

// ===========================================================================
// HostStore (POSIX shm, CPU compatibility path -- BASELINE config 1)
// ===========================================================================

struct HostVar : VarMeta {
    bool creator = false;
    std::string shm_name;
    std::vector<size_t> peer_bytes;
    std::vector<std::string> peer_names;
    at::Tensor goff;  // CPU int64 [ntotal+1], replicated
    int64_t oob_skipped = 0, cap_skipped = 0;
};

class HostStore {
public:
    HostStore(const std::string& session, int rank, int nparts)
        : session_(session), rank_(rank), nparts_(nparts) {
        TORCH_CHECK(nparts >= 1 && nparts <= DDS_MAX_PARTS,
                    "ddstore: world size must be in [1, ", DDS_MAX_PARTS, "]");
    }
    ~HostStore() {
        try { free_all(); } catch (...) {}
    }

    std::string shm_name(const std::string& var) const {
        return "/dds-" + session_ + "-" + var + "-" + std::to_string(rank_);
    }

    // The four registrations, as DeviceStore's; each returns the name of the
    // shard's shm segment.
    std::string add(const std::string& name, const at::Tensor& src, int64_t nrows,
                    int64_t row_elems, std::vector<int64_t> nrows_all) {
        return register_var(name, "add", &src, src.scalar_type(), row_elems, nrows,
                            nrows_all, nullptr);
    }

    std::string init(const std::string& name, int64_t nrows, int64_t row_elems,
                     at::ScalarType st, std::vector<int64_t> nrows_all) {
        return register_var(name, "init", nullptr, st, row_elems, nrows, nrows_all,
                            nullptr);
    }

    std::string add_csr(const std::string& name, const at::Tensor& values,
                        int64_t nsamples, int64_t nelems, int64_t row_elems,
                        std::vector<int64_t> nsamples_all,
                        std::vector<int64_t> nelems_all, const at::Tensor& goff_cpu) {
        const CsrShape csr{nelems, nelems_all, goff_cpu};
        return register_var(name, "add_csr", &values, values.scalar_type(), row_elems,
                            nsamples, nsamples_all, &csr);
    }

    std::string init_csr(const std::string& name, int64_t nsamples,
                         int64_t nelems, int64_t row_elems, at::ScalarType st,
                         std::vector<int64_t> nsamples_all,
                         std::vector<int64_t> nelems_all,
                         const at::Tensor& goff_cpu) {
        const CsrShape csr{nelems, nelems_all, goff_cpu};
        return register_var(name, "init_csr", nullptr, st, row_elems, nsamples,
                            nsamples_all, &csr);
    }

    void update(const std::string& name, const at::Tensor& src, int64_t offset) {
        fill(name, src, offset, false);
    }
    void update_elems(const std::string& name, const at::Tensor& src,
                      int64_t elem_offset) {
        fill(name, src, elem_offset, true);
    }

    void open_peers(const std::string& name, const std::vector<std::string>& names) {
        HostVar& v = var(name);
        TORCH_CHECK((int)names.size() == nparts_, "ddstore open_peers: size mismatch");
        v.peers.assign(nparts_, nullptr);
        v.peer_bytes.assign(nparts_, 0);
        v.peer_names = names;
        const std::vector<int64_t>& cnt_prefix = v.is_csr ? v.elem_prefix : v.prefix;
        for (int r = 0; r < nparts_; ++r) {
            size_t nb = (size_t)((cnt_prefix[r + 1] - cnt_prefix[r]) * v.row_elems *
                                 v.itemsize);
            if (nb < 1) nb = 1;
            if (r == rank_) {
                v.peers[r] = v.base;
                v.peer_bytes[r] = 0;  // not mapped, do not munmap
                continue;
            }
            int fd = shm_open(names[r].c_str(), O_RDONLY, 0600);
            TORCH_CHECK(fd >= 0, "ddstore: shm_open failed for ", names[r]);
            void* p = mmap(nullptr, nb, PROT_READ, MAP_SHARED, fd, 0);
            close(fd);
            TORCH_CHECK(p != MAP_FAILED, "ddstore: mmap failed for ", names[r]);
#if defined(MADV_HUGEPAGE)
            (void)madvise(p, nb, MADV_HUGEPAGE);
#endif
            try_collapse_hugepages(p, nb);  // peer VMA: PMD-map shared pages
            v.peers[r] = p;
            v.peer_bytes[r] = nb;
        }
    }

    void get_range(const std::string& name, int64_t start, int64_t count,
                   at::Tensor out) {
        HostVar& v = var(name);
        check_range_out(v, out, count, true);
        check_peers(v);
        const auto [src, nb] = owned_range(v, start, count);
        std::memcpy(out.data_ptr(), src, nb);
        v.count(count, (int64_t)nb);
    }

    void gather(const std::string& name, const at::Tensor& idx, at::Tensor out) {
        HostVar& v = var(name);
        TORCH_CHECK(!v.is_csr, "ddstore gather: use gather_csr for CSR variables");
        check_peers(v);
        TORCH_CHECK(idx.scalar_type() == at::kLong && idx.is_contiguous() &&
                        idx.device().is_cpu(),
                    "ddstore gather: indices must be contiguous int64 on CPU");
        int64_t nidx = idx.numel();
        // dtype (not just itemsize) must match: a same-size different dtype
        // (bf16 out from an f16 store) would silently bit-reinterpret here
        // while the GPU path converts numerically; the Python
        // layer converts via a staging tensor when dtypes differ.
        TORCH_CHECK(out.is_contiguous() && out.device().is_cpu() &&
                        dds_type_of(out) == v.dds_t,
                    "ddstore gather: output must be a contiguous CPU tensor of the store dtype");
        TORCH_CHECK(out.numel() == nidx * v.row_elems, "ddstore gather: shape mismatch");
        const int64_t* ip = idx.data_ptr<int64_t>();
        const int64_t rb = v.row_elems * v.itemsize;
        char* op = (char*)out.data_ptr();
        const int64_t ntotal = v.prefix[nparts_];
        // random source rows are DRAM-latency-bound: software-prefetch the
        // row PF iterations ahead (the extra owner lookup is ~free), and
        // write the packed output with non-temporal stores
        const int64_t PF = host_prefetch_dist();
        host_parallel_for(0, nidx, 1024, [&](int64_t b, int64_t e) {
            auto src_of = [&](int64_t g) -> const char* {
                int p = owner_of_host(v.prefix, g);
                return (const char*)v.peers[p] + (g - v.prefix[p]) * rb;
            };
            for (int64_t i = b; i < e; ++i) {
                if (PF > 0 && i + PF < e) {
                    int64_t gp = ip[i + PF];
                    if (gp >= 0 && gp < ntotal) {
                        const char* ps = src_of(gp);
                        for (int64_t o = 0; o < rb; o += 64)
                            __builtin_prefetch(ps + o, 0, 1);
                    }
                }
                int64_t g = ip[i];
                TORCH_CHECK(g >= 0 && g < ntotal, "ddstore gather: index out of range");
                copy_row_nt(op + i * rb, src_of(g), (size_t)rb);
            }
        });
        copy_rows_fence();
        v.count(nidx, nidx * rb);
    }

    void gather_csr(const std::string& name, const at::Tensor& idx,
                    const at::Tensor& out_off, at::Tensor out, int64_t total_elems) {
        HostVar& v = var(name);
        TORCH_CHECK(v.is_csr, "ddstore gather_csr: not a CSR variable");
        check_peers(v);
        TORCH_CHECK(idx.scalar_type() == at::kLong && idx.is_contiguous() &&
                        idx.device().is_cpu(), "ddstore gather_csr: bad indices");
        TORCH_CHECK(out_off.scalar_type() == at::kLong && out_off.is_contiguous() &&
                        out_off.numel() == idx.numel() + 1,
                    "ddstore gather_csr: bad out_off");
        TORCH_CHECK(out.is_contiguous() && out.device().is_cpu() &&
                        dds_type_of(out) == v.dds_t &&
                        out.numel() >= total_elems * v.row_elems,
                    "ddstore gather_csr: bad output tensor");
        const int64_t* ip = idx.data_ptr<int64_t>();
        const int64_t* oo = out_off.data_ptr<int64_t>();
        const int64_t* go = v.goff.data_ptr<int64_t>();
        const int64_t eb = v.row_elems * v.itemsize;
        const int64_t ntotal = v.prefix[nparts_];
        // real buffer capacity in elements: a sample whose slice would end
        // past it (or an out-of-range id) is skipped + counted, mirroring
        // the device kernels -- never read/written out of bounds
        const int64_t cap =
            out.numel() / (v.row_elems > 0 ? v.row_elems : (int64_t)1);
        char* op = (char*)out.data_ptr();
        std::atomic<int64_t> oob(0), capskip(0), elems(0);
        host_parallel_for(0, idx.numel(), 64, [&](int64_t b, int64_t e) {
            int64_t my_oob = 0, my_cap = 0, my_elems = 0;
            for (int64_t s = b; s < e; ++s) {
                int64_t g = ip[s];
                if (g < 0 || g >= ntotal) {
                    ++my_oob;
                    continue;
                }
                int p = owner_of_host(v.prefix, g);
                int64_t e0 = go[g], n = go[g + 1] - go[g];
                if (n <= 0) continue;  // an empty sample: nothing to write or skip
                if (oo[s] < 0 || oo[s] + n > cap) {
                    ++my_cap;
                    continue;
                }
                std::memcpy(op + oo[s] * eb,
                            (const char*)v.peers[p] + (e0 - v.elem_prefix[p]) * eb,
                            (size_t)(n * eb));
                my_elems += n;
            }
            oob += my_oob;
            capskip += my_cap;
            elems += my_elems;
        });
        v.oob_skipped += oob.load();
        v.cap_skipped += capskip.load();
        v.count(idx.numel(), elems.load() * eb);  // true gathered bytes
    }

    void scatter_local(const std::string& name, const at::Tensor& local_idx,
                       const at::Tensor& src) {
        HostVar& v = var(name);
        TORCH_CHECK(!v.is_csr, "ddstore scatter_local: CSR not supported");
        TORCH_CHECK(local_idx.scalar_type() == at::kLong && local_idx.is_contiguous() &&
                        local_idx.device().is_cpu(), "ddstore scatter_local: bad indices");
        TORCH_CHECK(src.is_contiguous() && src.device().is_cpu() &&
                        dds_type_of(src) == v.dds_t &&
                        src.numel() == local_idx.numel() * v.row_elems,
                    "ddstore scatter_local: bad src");
        const int64_t* ip = local_idx.data_ptr<int64_t>();
        const int64_t rb = v.row_elems * v.itemsize;
        const char* sp = (const char*)src.data_ptr();
        host_parallel_for(0, local_idx.numel(), 1024, [&](int64_t b, int64_t e) {
            for (int64_t i = b; i < e; ++i) {
                TORCH_CHECK(ip[i] >= 0 && ip[i] < v.nrows_local,
                            "ddstore scatter_local: index out of range");
                std::memcpy((char*)v.base + ip[i] * rb, sp + i * rb, (size_t)rb);
            }
        });
    }

    at::Tensor local_shard(const std::string& name) {
        HostVar& v = var(name);
        return at::from_blob(v.base, {v.local_count(), v.row_elems},
                             at::TensorOptions().dtype(v.st));
    }

    void epoch_begin() { fsm_.begin(); }
    void epoch_end() {
        fsm_.end();
        if (strict_mode()) check_strict();
    }
    bool epoch_active() const { return fsm_.fence_active; }

    void check_strict() {
        for (auto& kv : vars_)
            strict_check(kv.first, kv.second.oob_skipped, kv.second.cap_skipped);
    }

    void reset_counters(const std::string& name) {
        HostVar& v = var(name);
        v.oob_skipped = v.cap_skipped = 0;
        v.n_gather = v.rows_gathered = v.bytes_gathered = 0;
    }

    py::dict query(const std::string& name) {
        HostVar& v = var(name);
        py::dict d = query_layout(v);
        d["bytes_gathered"] = v.bytes_gathered;
        d["oob_skipped"] = v.oob_skipped;
        d["cap_skipped"] = v.cap_skipped;
        return d;
    }

    bool has(const std::string& name) const { return vars_.count(name) > 0; }

    void free_var(const std::string& name) {
        auto it = vars_.find(name);
        TORCH_CHECK(it != vars_.end(), "ddstore: unknown variable '", name, "'");
        release(it->second);
        vars_.erase(it);
    }

    void free_all() {
        for (auto& kv : vars_) release(kv.second);
        vars_.clear();
    }

private:
    void check_new(const std::string& name) {
        TORCH_CHECK(!vars_.count(name), "ddstore: variable '", name, "' already exists");
    }
    HostVar& var(const std::string& name) {
        auto it = vars_.find(name);
        TORCH_CHECK(it != vars_.end(), "ddstore: unknown variable '", name, "'");
        return it->second;
    }
    void check_peers(const HostVar& v) {
        TORCH_CHECK(!v.peers.empty(),
                    "ddstore: variable not finalized (open_peers not called)");
    }

    void create_shm(HostVar& v, const std::string& name, size_t bytes) {
        v.shm_name = shm_name(name);
        TORCH_CHECK(v.shm_name.size() < 250, "ddstore: variable name too long");
        v.base_bytes = bytes < 1 ? 1 : bytes;
        shm_unlink(v.shm_name.c_str());  // stale segment from a crashed run
        int fd = shm_open(v.shm_name.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
        TORCH_CHECK(fd >= 0, "ddstore: shm_open(create) failed for ", v.shm_name);
        int rc = ftruncate(fd, (off_t)v.base_bytes);
        if (rc != 0) {
            close(fd);
            shm_unlink(v.shm_name.c_str());
            TORCH_CHECK(false, "ddstore: ftruncate failed (shm too large?)");
        }
        v.base = mmap(nullptr, v.base_bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        close(fd);
        TORCH_CHECK(v.base != MAP_FAILED, "ddstore: mmap failed");
#if defined(MADV_HUGEPAGE)
        // shm defaults to 4-KB pages; where shmem THP is enabled ("advise")
        // this collapses the random-gather TLB pressure
        (void)madvise(v.base, v.base_bytes, MADV_HUGEPAGE);
#endif
        v.creator = true;
    }

    void release(HostVar& v) {
        for (size_t r = 0; r < v.peers.size(); ++r)
            if (v.peer_bytes[r] > 0 && v.peers[r]) munmap(v.peers[r], v.peer_bytes[r]);
        v.peers.clear();
        if (v.base && v.base != MAP_FAILED) munmap(v.base, v.base_bytes);
        if (v.creator) shm_unlink(v.shm_name.c_str());
        v.base = nullptr;
    }

    // The one registration body (arguments as describe_var): create the shm
    // segment and fill it from `src` or with zeros.
    std::string register_var(const std::string& name, const char* op,
                             const at::Tensor* src, at::ScalarType st, int64_t row_elems,
                             int64_t n_local, const std::vector<int64_t>& counts,
                             const CsrShape* csr) {
        check_new(name);
        HostVar v;
        describe_var(v, op, src, st, row_elems, n_local, counts, csr, true);
        if (csr) v.goff = csr->goff;
        create_shm(v, name, v.shard_bytes());
        if (src)
            std::memcpy(v.base, src->data_ptr(), (size_t)src->numel() * v.itemsize);
        else
            std::memset(v.base, 0, v.base_bytes);
        try_collapse_hugepages(v.base, v.base_bytes);
        std::string n = v.shm_name;
        vars_[name] = std::move(v);
        return n;
    }

    // body of update and update_elems
    void fill(const std::string& name, const at::Tensor& src, int64_t offset, bool elems) {
        HostVar& v = var(name);
        const int64_t at = check_update(v, elems, src, offset, true);
        std::memcpy((char*)v.base + at, src.data_ptr(), (size_t)src.numel() * v.itemsize);
    }

    std::string session_;
    int rank_;
    int nparts_;
    EpochFSM fsm_;
    std::map<std::string, HostVar> vars_;
};

// ===========================================================================
// Cycle traversal of a permutation (host): the in-place chunked reshuffle
// processes slots in cycle order so a bounded buffer suffices -- slot j_i is
// written from slot j_{i+1}=perm[j_i]'s OLD row, and within a contiguous
// cycle traversal every read slot is only overwritten at the same or a later
// position. Returns (order[n], starts[ncycles+1]): `order` is the
// concatenated cycle traversal, `starts` its cycle start positions
// (starts[ncycles] = n). Single O(n) pointer-chasing walk.
// ===========================================================================
template <typename I>
inline void cycle_walk(const I* p, int64_t n, int64_t* order,
                       std::vector<int64_t>& starts) {
    // the walk is a dependent random-access chain (unprefetchable); a
    // 32-bit working copy halves its memory traffic for n < 2^31
    std::vector<bool> visited((size_t)n, false);
    int64_t w = 0;
    for (int64_t s0 = 0; s0 < n; ++s0) {
        if (visited[(size_t)s0]) continue;
        starts.push_back(w);
        int64_t j = s0;
        while (!visited[(size_t)j]) {
            visited[(size_t)j] = true;
            order[w++] = j;
            j = (int64_t)p[j];
            TORCH_CHECK(j >= 0 && j < n,
                        "ddstore cycle_order: not a permutation (value out of range)");
        }
        TORCH_CHECK(j == s0,
                    "ddstore cycle_order: not a permutation (duplicate value)");
    }
}

inline std::pair<at::Tensor, at::Tensor> cycle_order(const at::Tensor& perm) {
    TORCH_CHECK(perm.scalar_type() == at::kLong && perm.is_contiguous() &&
                    perm.device().is_cpu(),
                "ddstore cycle_order: perm must be a contiguous int64 CPU tensor");
    const int64_t n = perm.numel();
    const int64_t* p = perm.data_ptr<int64_t>();
    at::Tensor order_t = at::empty({n}, at::TensorOptions().dtype(at::kLong));
    int64_t* order = order_t.data_ptr<int64_t>();
    std::vector<int64_t> starts;
    if (n <= (int64_t)INT32_MAX) {
        std::vector<int32_t> p32((size_t)n);
        host_parallel_for(0, n, 1 << 20, [&](int64_t b, int64_t e) {
            for (int64_t i = b; i < e; ++i) p32[(size_t)i] = (int32_t)p[i];
        });
        cycle_walk(p32.data(), n, order, starts);
    } else {
        cycle_walk(p, n, order, starts);
    }
    starts.push_back(n);
    at::Tensor starts_t = at::empty({(int64_t)starts.size()},
                                    at::TensorOptions().dtype(at::kLong));
    std::memcpy(starts_t.data_ptr<int64_t>(), starts.data(),
                starts.size() * sizeof(int64_t));
    return {order_t, starts_t};
}

} // namespace ddstore


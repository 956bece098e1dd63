// aps_internal.h — shared plumbing of libaps_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/aps.h"

namespace aps {

// ---- error transport ---------------------------------------------------------------------------
struct Error : std::exception {
    int code;
    std::string msg;
    Error(int c, std::string m) : code(c), msg(std::move(m)) {}
    const char* what() const noexcept override { return msg.c_str(); }
};

[[noreturn]] void fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
void set_last_error(const char* s);

#define APS_HIP(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            ::aps::fail(e_ == hipErrorOutOfMemory ? APS_E_OOM : APS_E_DEVICE,               \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,    \
                        __LINE__);                                                          \
    } while (0)

#define APS_REQUIRE(cond, code, ...)                   \
    do {                                               \
        if (!(cond)) ::aps::fail((code), __VA_ARGS__); \
    } while (0)

// Wraps the body of every extern "C" entry point.
template <class F>
inline int guarded(F&& f) {
    try {
        f();
        return APS_OK;
    } catch (const Error& e) {
        set_last_error(e.msg.c_str());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("host allocation failed");
        return APS_E_OOM;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return APS_E_INTERNAL;
    } catch (...) {
        set_last_error("unknown exception");
        return APS_E_INTERNAL;
    }
}

// ---- per-thread context --------------------------------------------------------------------------
struct Ctx {
    int device = -1;
    hipStream_t own_stream = nullptr;
    hipStream_t user_stream = nullptr;
    bool use_user_stream = false;
    int own_priority = 0;  // 1: own_stream was created at the device's highest priority
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    struct Block {
        void* p;
        size_t bytes;
        bool used;
    };
    std::vector<Block> blocks;
    hipStream_t stream() const { return use_user_stream ? user_stream : own_stream; }
};

// Makes sure a gfx950 device is selected for this thread and returns the context.
Ctx& ctx();
inline hipStream_t stream() { return ctx().stream(); }

// Cached device workspace (hipMalloc is synchronising; steady state must not call it).
void* ws_alloc(size_t bytes);
void ws_free(void* p);
// Bytes of this thread's cached blocks that are not in use (device memory a new request can be served from).
size_t ws_idle_bytes();

template <class T>
struct Ws {
    T* p = nullptr;
    size_t n = 0;
    Ws() = default;
    explicit Ws(size_t count) { alloc(count); }
    Ws(const Ws&) = delete;
    Ws& operator=(const Ws&) = delete;
    Ws(Ws&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; }
    Ws& operator=(Ws&& o) noexcept {
        if (this != &o) {
            reset();
            p = o.p;
            n = o.n;
            o.p = nullptr;
        }
        return *this;
    }
    ~Ws() { reset(); }
    void alloc(size_t count) {
        reset();
        n = count;
        p = static_cast<T*>(ws_alloc((count ? count : 1) * sizeof(T)));
    }
    void reset() {
        if (p) ws_free(p);
        p = nullptr;
    }
    T* get() const { return p; }
    operator T*() const { return p; }
};

// ---- host/device pointer staging -----------------------------------------------------------------
bool is_device_ptr(const void* p);

// Input that may live on the host: gives a device pointer valid until destruction.
template <class T>
struct In {
    const T* d = nullptr;
    Ws<T> tmp;
    In() = default;
    In(const T* p, size_t count) { bind(p, count); }
    void bind(const T* p, size_t count) {
        if (count == 0 || p == nullptr) {
            d = p;
            return;
        }
        if (is_device_ptr(p)) {
            d = p;
        } else {
            tmp.alloc(count);
            APS_HIP(hipMemcpyAsync(tmp.p, p, count * sizeof(T), hipMemcpyHostToDevice, stream()));
            d = tmp.p;
        }
    }
    const T* get() const { return d; }
    operator const T*() const { return d; }
};

// Output that may live on the host: device pointer now, copied back by commit().
template <class T>
struct Out {
    T* d = nullptr;
    T* host = nullptr;
    size_t n = 0;
    Ws<T> tmp;
    Out() = default;
    Out(T* p, size_t count) { bind(p, count); }
    void bind(T* p, size_t count) {
        n = count;
        if (p == nullptr) return;
        if (count == 0 || is_device_ptr(p)) {
            d = p;
        } else {
            host = p;
            tmp.alloc(count);
            d = tmp.p;
        }
    }
    // Copies back `count` elements (default: all).  Synchronises when the target is host memory.
    void commit(size_t count = SIZE_MAX) {
        if (!host) return;
        if (count > n) count = n;
        if (count) {
            APS_HIP(hipMemcpyAsync(host, d, count * sizeof(T), hipMemcpyDeviceToHost, stream()));
            APS_HIP(hipStreamSynchronize(stream()));
        }
    }
    // Copies back `rows` runs of `width` elements that lie `ld` elements apart (a matrix with a caller-given leading
    // dimension): the elements between the runs belong to the caller and are not written, as with a device target.
    void commit_2d(size_t width, size_t rows, size_t ld) {
        if (!host || width == 0 || rows == 0) return;
        if (ld == width || rows == 1) return commit(width * rows);
        APS_HIP(hipMemcpy2DAsync(host, ld * sizeof(T), d, ld * sizeof(T), width * sizeof(T), rows, hipMemcpyDeviceToHost, stream()));
        APS_HIP(hipStreamSynchronize(stream()));
    }
    T* get() const { return d; }
    operator T*() const { return d; }
    bool present() const { return d != nullptr; }
};

// Scoped event bracket around a kernel launch site (no-op unless aps_profile_enable(1)).
struct Prof {
    int slot = -1;
    void* ev_b = nullptr;
    explicit Prof(const char* name);
    ~Prof();
};

inline void check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) fail(APS_E_DEVICE, "launch of %s failed: %s", what, hipGetErrorString(e));
}

// elements a matrix of n rows x cols columns spans under a leading dimension (n > 0)
inline size_t matrix_extent(int64_t n, int64_t ld, int64_t cols, int layout) {
    return layout == APS_ROWMAJOR ? (size_t)(n - 1) * ld + cols : (size_t)(cols - 1) * ld + n;
}

// the largest j in [0, n) with off(j) <= key, for ascending off with off(0) <= key: the segment a row, a tile or a block lies in
template <class Off, class Key>
__device__ __forceinline__ int last_at_or_below_by(Off&& off, int n, Key key) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off(mid) <= key) lo = mid; else hi = mid - 1;
    }
    return lo;
}
template <class T, class Key>
__device__ __forceinline__ int last_at_or_below(const T* __restrict__ off, int n, Key key) {
    return last_at_or_below_by([off](int j) { return off[j]; }, n, key);
}

// The (row, column set) slot table of the global k-NN (match.hip): the rows of set i against set j own the slots
// job_off[i n + j] + local row.  every_j: the pooled matcher's form - every j, the diagonal too, for the query sets
// [a, b) (the other sets' entries are 0); otherwise the blocked form - different sets only, -1 on the diagonal.
struct SlotTable {
    std::vector<int64_t> job_off;
    int64_t slots = 0;
};
SlotTable slot_table(const std::vector<int64_t>& off, int a, int b, bool every_j);
// match.hip: the screening half of the blocked global k-NN (see the definition)
void screened_block_top3(const float* X_dev, int64_t ld, int layout, const std::vector<int64_t>& block_off, const SlotTable& table,
                         uint32_t* t3_idx, float* t3_d, float* t3_b);
// The images' prepared operand forms and their stats (match.hip): the first pass of a search builds them, the later ones
// reuse them, the destructor releases them.
struct GlobalSets {
    struct Impl;
    Impl* impl = nullptr;
    GlobalSets() = default;
    GlobalSets(const GlobalSets&) = delete;
    GlobalSets& operator=(const GlobalSets&) = delete;
    ~GlobalSets();
};
// The pooled matcher's search with featureMatchingGlobal's filter in view (match.hip), for the query images [img_a, img_b):
// rows the filter provably drops at `ratio` are flagged in dismissed[] and not searched; for the others t3_* hold, per
// (row, image) slot, the certified prefix of the three nearest rows of that image and the bound of its unlisted rows.
// Returns the rows that survive phase 0's proof.
int64_t screened_global_top3(const float* X_dev, int64_t ld, int layout, const std::vector<int64_t>& img_off, int img_a, int img_b,
                             float ratio, const SlotTable& table, const int64_t* d_img_off, const int64_t* d_job_off, GlobalSets& sets,
                             uint32_t* t3_idx, float* t3_d, float* t3_b, uint8_t* dismissed);

// surf.hip: select_dev.h's selection and ordered compaction for a translation unit that builds the keys of its own int4 candidates
// (kaze.hip).  The selection's kernels are instantiated in every translation unit that launches them; a detector whose candidates
// are SURF's records runs surf.hip's copies instead of carrying a fourth set.  One group of n candidates (keys below 2^60), of which
// `keep` <= n stay: cells == 0 by (key ascending, index ascending), keys of 32 bits (select_by_key); cells > 0 spread over the
// segments key >> 32 < cells by water-filling (select_uniform's composite-key form).  sel[0 .. keep - 1] = the kept candidates in
// the order they had; *d_kept = the number the device kept.  On the calling thread's stream; no read-back.
void select_int4_group(const unsigned long long* keys, const unsigned int* vals, const int4* cand, unsigned int n, unsigned int keep,
                       unsigned int cells, int4* sel, unsigned int* d_kept);

// set bits of a 64-bit ballot word, as a rocprim transform (surf.hip, fast.hip, hamming_pairs.hip: the scans behind their ordered compactions)
struct PopcOp {
    __host__ __device__ unsigned int operator()(unsigned long long v) const {
#if defined(__HIP_DEVICE_COMPILE__)
        return (unsigned int)__popcll(v);
#else
        return (unsigned int)__builtin_popcountll(v);
#endif
    }
};

inline unsigned cdiv(size_t a, size_t b) { return static_cast<unsigned>((a + b - 1) / b); }

// compile-time loop: the body receives std::integral_constant<int, I>, so register arrays are indexed by constants
// by construction (an index the optimiser fails to fold sends the whole array to scratch memory)
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}


}  // namespace aps

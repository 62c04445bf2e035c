// values.hip -- sblas_csr_set_values: new values for a handle's entries with
// the pattern, every analysed SpMV plan, AUTO's choice and the deterministic
// mode kept.
//
// Every plan that copies values holds a fixed permutation of the CSR value
// array plus zero padding: the xsort chunk storage, the XCD-panel CSR
// (PanelPlan::val; ROWSPLIT's panel form runs on it too) and the CSR5 tiles.
// For each such buffer the handle keeps a source-index map -- per value slot
// the int32 index into the CSR values, -1 for padding -- and a refresh is one
// pull pass over it (k_sv_gather): dst[slot] = map[slot] >= 0 ?
// d_val[map[slot]] : 0.0, two slots per thread, 16-B stores.  CSR5's plain
// form needs no map: its tile transposition is a closed formula
// (k_sv_c5_tiles).  ROWSPLIT reads A.val directly.
//
// The maps are built by the first call after a plan's analysis and kept with
// the plan.  A map is derived by running the plan's own placement code over an
// index payload: a double array shaped like A.val holding i + 1 at entry i
// (exact in fp64) and 0.0 in the padding.  Whatever the placement writes to a
// value slot then names the slot's source (0.0, the padding, gives -1), so a
// map agrees with its layout builder by construction: the host-built and the
// device-built xsort layout, which are byte-identical, give the same map, and
// duplicate (row, column) entries keep the stable order of the sort.
// When a map cannot be allocated (test option "sv_map_nomem") the plan is
// freed and rebuilt from the new values in the same form.
//
// The SpMM plan merges duplicate entries into its fragments: it is dropped
// and rebuilt by the next sblas_spmm.
#include <algorithm>
#include <chrono>
#include <memory>
#include <vector>

#include "sblas_internal.hpp"

namespace sblas {

namespace {

// slot s of a buffer stored in runs of 2^seg_shift slots, `stride` doubles apart
__device__ __forceinline__ long long sv_slot(long long s, int seg_shift, long long stride)
{
    const long long c = s >> seg_shift;
    return c * stride + (s - (c << seg_shift));
}

__global__ __launch_bounds__(256) void k_sv_gather(double *__restrict__ dst, const int *__restrict__ map,
                                                   const double *__restrict__ src, long long nnz,
                                                   long long npairs, int seg_shift, long long stride)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npairs) return;
    const int2 mm = reinterpret_cast<const int2 *>(map)[i];
    double2 v;
    v.x = mm.x >= 0 && mm.x < nnz ? src[mm.x] : 0.0;
    v.y = mm.y >= 0 && mm.y < nnz ? src[mm.y] : 0.0;
    *reinterpret_cast<double2 *>(dst + sv_slot(2 * i, seg_shift, stride)) = v;
}

__global__ __launch_bounds__(256) void k_sv_payload(double *__restrict__ p, long long nnz, long long cap)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < cap) p[i] = i < nnz ? (double)(i + 1) : 0.0;
}

__global__ __launch_bounds__(256) void k_sv_map(const double *__restrict__ pv, long long nslots, int seg_shift,
                                                long long stride, int *__restrict__ map)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nslots) map[i] = (int)pv[sv_slot(i, seg_shift, stride)] - 1;
}

// CSR5's tile transposition (spmv.hip c5_vpos) in pull form, a pair of slots
// per thread: slot o = (k/2)*128 + 2l + (k&1) of tile t holds entry
// t*1024 + l*16 + k.  T = double: the values; T = int: a map from a payload.
template <class T>
__device__ __forceinline__ T sv_conv(double v);
template <>
__device__ __forceinline__ double sv_conv<double>(double v)
{
    return v;
}
template <>
__device__ __forceinline__ int sv_conv<int>(double v)
{
    return (int)v - 1;
}

template <class T>
struct SvPair;  // two adjacent slots, stored as one word
template <>
struct SvPair<double> {
    typedef double2 type;
};
template <>
struct SvPair<int> {
    typedef int2 type;
};

template <class T>
__global__ __launch_bounds__(256) void k_sv_c5_tiles(T *__restrict__ out, const double *__restrict__ val,
                                                     long long nnz, long long npairs)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npairs) return;
    const long long o = 2 * i, t = o / kC5Tile;
    const int w = (int)(o - t * kC5Tile);
    const int l = (w & 127) >> 1, k = (w >> 7) * 2;
    const long long e = t * kC5Tile + (long long)l * kC5Sigma + k;
    typename SvPair<T>::type v;
    v.x = sv_conv<T>(e < nnz ? val[e] : 0.0);
    v.y = sv_conv<T>(e + 1 < nnz ? val[e + 1] : 0.0);
    *reinterpret_cast<typename SvPair<T>::type *>(out + o) = v;  // o is even: the pair is aligned
}

unsigned sv_grid(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

int *sv_map_alloc(long long nslots)
{
    double opt = 0.0;
    if (test_option("sv_map_nomem", &opt) && opt != 0.0) return nullptr;
    int *p = nullptr;
    if (hipMalloc(&p, sizeof(int) * (size_t)std::max<long long>(nslots, 1)) != hipSuccess) {
        (void)hipGetLastError();  // not an error of the call: the plan is rebuilt instead
        return nullptr;
    }
    return p;
}

int sv_map_from_payload(const double *pv, long long nslots, int seg_shift, long long stride, int *map,
                        hipStream_t s)
{
    if (nslots <= 0) return SBLAS_OK;
    hipLaunchKernelGGL(k_sv_map, dim3(sv_grid(nslots)), dim3(256), 0, s, pv, nslots, seg_shift, stride, map);
    SBLAS_HIP(hipGetLastError());
    return SBLAS_OK;
}

int sv_gather(double *dst, const int *map, const double *src, long long nnz, long long nslots, int seg_shift,
              long long stride, hipStream_t s)
{
    if (nslots <= 0) return SBLAS_OK;
    SBLAS_LAUNCH(k_sv_gather, dim3(sv_grid(nslots / 2)), dim3(256), 0, s, dst, map, src, nnz, nslots / 2,
                 seg_shift, stride);
    SBLAS_HIP(hipGetLastError());
    return SBLAS_OK;
}

int sv_c5_tiles(double *tval, const double *val, long long nnz, long long ntiles, hipStream_t s)
{
    const long long npairs = ntiles * kC5Tile / 2;
    if (npairs <= 0) return SBLAS_OK;
    SBLAS_LAUNCH(k_sv_c5_tiles<double>, dim3(sv_grid(npairs)), dim3(256), 0, s, tval, val, nnz, npairs);
    SBLAS_HIP(hipGetLastError());
    return SBLAS_OK;
}

int sv_c5_tiles_map(int *map, const double *pv, long long nnz, long long ntiles, hipStream_t s)
{
    const long long npairs = ntiles * kC5Tile / 2;
    if (npairs <= 0) return SBLAS_OK;
    hipLaunchKernelGGL(k_sv_c5_tiles<int>, dim3(sv_grid(npairs)), dim3(256), 0, s, map, pv, nnz, npairs);
    SBLAS_HIP(hipGetLastError());
    return SBLAS_OK;
}

namespace {

constexpr int kXsSegShift = 8;                                // 256 value slots per chunk ...
constexpr long long kXsSegStride = kXsChunkBytes / sizeof(double);  // ... every 3072 B

// The xsort map: the layout builder that built the plan (device or host) run
// once more over the payload into a scratch copy of the chunk storage, whose
// value slots then name their sources.  Waits for the device, as analyse does.
int xs_value_map(sblas_csr_s &A, const double *payload, hipStream_t s, int *map)
{
    XsPlan &P = A.xs;
    // the builders read A.val and publish into A.xs.key: lend them the payload
    // and an empty slot, and put the handle back whatever they return
    double *const keep_val = A.val;
    uint32_t *const keep_key = P.key;
    const long long keep_d2h = P.d2h_bytes, keep_scratch = P.scratch_bytes;
    A.val = const_cast<double *>(payload);
    P.key = nullptr;
    std::vector<long long> blk;
    std::unique_ptr<unsigned char[]> hbuf;
    bool on_device = P.dev_built;
    int st = SBLAS_OK;
    if (on_device) st = xs_layout_device(A, P.h_ranges, P.rows_cap, P.nrows_cap, s, blk, on_device);
    if (st == SBLAS_OK && !on_device) st = xs_layout_host(A, P.h_ranges, P.rows_cap, P.nrows_cap, blk, hbuf);
    unsigned char *tmp = reinterpret_cast<unsigned char *>(P.key);
    A.val = keep_val;
    P.key = keep_key;
    P.d2h_bytes = keep_d2h;
    P.scratch_bytes = keep_scratch;
    if (st == SBLAS_OK && (blk.empty() || blk.back() != P.nchunks)) {
        set_error("set_values: the value map's layout has %lld chunks, the plan %lld",
                  blk.empty() ? -1LL : blk.back(), P.nchunks);
        st = SBLAS_ERR_HIP;
    }
    const size_t nb = (size_t)P.nchunks * kXsChunkBytes;
    if (st == SBLAS_OK && !on_device) {
        hipError_t e = hipMalloc(&tmp, nb);
        if (e == hipSuccess) e = hipMemcpy(tmp, hbuf.get(), nb, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            set_error("set_values: xsort value map: %s", hipGetErrorString(e));
            st = SBLAS_ERR_HIP;
        }
    }
    if (st == SBLAS_OK)
        st = sv_map_from_payload(reinterpret_cast<const double *>(tmp + kXsChunk * sizeof(uint32_t)),
                                 P.nchunks * kXsChunk, kXsSegShift, kXsSegStride, map, s);
    if (st == SBLAS_OK && hipStreamSynchronize(s) != hipSuccess) {
        set_error("set_values: xsort value map: %s", hipGetErrorString(hipGetLastError()));
        st = SBLAS_ERR_HIP;
    }
    (void)hipFree(tmp);
    return st;
}

long long c5_map_bytes(const Csr5Plan &P)
{
    long long b = P.vmap ? (long long)sizeof(int) * P.ntiles * kC5Tile : 0;
    for (const Csr5Plan &Q : P.panels) b += c5_map_bytes(Q);
    return b;
}

bool c5_needs_map(const Csr5Plan &P)
{
    if (!P.ready || P.P == 0) return false;
    for (const Csr5Plan &Q : P.panels)
        if (Q.ntiles && !Q.vmap) return true;
    return false;
}

}  // namespace

int sv_refresh_xsort(sblas_csr_s &A, const double *d_val, const double *payload, hipStream_t s, bool *rebuilt)
{
    XsPlan &P = A.xs;
    if (!P.ready || P.nchunks == 0) return SBLAS_OK;
    if (!P.vmap) {
        int *map = payload ? sv_map_alloc(P.nchunks * kXsChunk) : nullptr;
        if (!map) {  // no room for a map: the plan again, from the new values
            free_xsort_plan(A);
            *rebuilt = true;
            return build_xsort_plan(A, s);
        }
        const int st = xs_value_map(A, payload, s, map);
        if (st != SBLAS_OK) {
            (void)hipFree(map);
            return st;
        }
        P.vmap = map;
    }
    return sv_gather(P.val, P.vmap, d_val, A.nnz, P.nchunks * kXsChunk, kXsSegShift, kXsSegStride, s);
}

}  // namespace sblas

using namespace sblas;

extern "C" {

int sblas_csr_set_values(sblas_csr A, const double *d_val, void *stream)
{
    if (!A || (A->nnz > 0 && !d_val)) return SBLAS_ERR_INVALID;
    DeviceGuard g(A->device);
    hipStream_t s = (hipStream_t)stream;
    ++A->sv_calls;
    A->sv_rebuilt = false;
    A->sv_dropped_mm = false;
    if (A->mm.ready) {  // duplicates are merged in its fragments: rebuilt by the next sblas_spmm
        free_spmm_plan(*A);
        A->spmm_last[0] = A->spmm_last[1] = A->spmm_last[2] = -1;
        A->sv_dropped_mm = true;
    }
    const long long nnz = A->nnz;
    if (nnz == 0) return SBLAS_OK;
    // the first call after an analysis: the index payload for the maps still missing
    const bool need_map = (A->pn.ready && !A->pn.degenerate && !A->pn.vmap) || c5_needs_map(A->c5) ||
                          (A->xs.ready && A->xs.nchunks && !A->xs.vmap);
    const auto t0 = std::chrono::steady_clock::now();
    double *payload = nullptr;
    double opt = 0.0;
    if (need_map && !(test_option("sv_map_nomem", &opt) && opt != 0.0)) {
        const long long cap = ((nnz + 3) & ~3LL) + 4;  // A.val's shape (capi.hip alloc_padded)
        if (hipMalloc(&payload, sizeof(double) * (size_t)cap) != hipSuccess) {
            (void)hipGetLastError();
            payload = nullptr;  // the plans are rebuilt instead
        } else {
            hipLaunchKernelGGL(k_sv_payload, dim3(sv_grid(cap)), dim3(256), 0, s, payload, nnz, cap);
            // the host layout build and the panel split read it outside the stream
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) {
                (void)hipFree(payload);
                set_error("set_values: index payload: %s", hipGetErrorString(e));
                return SBLAS_ERR_HIP;
            }
        }
    }
    int st = SBLAS_OK;
    if (hipMemcpyAsync(A->val, d_val, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, s) != hipSuccess) {
        set_error("set_values: %s", hipGetErrorString(hipGetLastError()));
        st = SBLAS_ERR_HIP;
    }
    bool rebuilt = false;
    if (st == SBLAS_OK) st = sv_refresh_panel(*A, d_val, payload, s, &rebuilt);
    if (st == SBLAS_OK) st = sv_refresh_csr5(*A, d_val, payload, s, &rebuilt);
    if (st == SBLAS_OK) st = sv_refresh_xsort(*A, d_val, payload, s, &rebuilt);
    if (need_map) {
        // every map build has waited for its kernels: nothing reads the payload any more
        (void)hipFree(payload);
        if (st == SBLAS_OK && !rebuilt)
            A->sv_build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    A->sv_rebuilt = rebuilt;
    return st;
}

int sblas_csr_values_info(sblas_csr A, double *info)
{
    if (!A || !info) return SBLAS_ERR_INVALID;
    const long long pn_b = A->pn.vmap ? (long long)sizeof(int) * A->pn.vcap : 0;
    const long long c5_b = c5_map_bytes(A->c5);
    const long long xs_b = A->xs.vmap ? (long long)sizeof(int) * A->xs.nchunks * kXsChunk : 0;
    int mask = 0;
    if (pn_b && A->rs.ready && A->rs.panels) mask |= 1 << SBLAS_SPMV_ROWSPLIT;
    if (c5_b) mask |= 1 << SBLAS_SPMV_CSR5;
    if (pn_b) mask |= 1 << SBLAS_SPMV_PANEL;
    if (xs_b) mask |= 1 << SBLAS_SPMV_XSORT;
    info[0] = (double)A->sv_calls;
    info[1] = (double)mask;
    info[2] = (double)(pn_b + c5_b + xs_b);
    info[3] = A->sv_build_s;
    info[4] = A->sv_rebuilt ? 1.0 : 0.0;
    info[5] = A->sv_dropped_mm ? 1.0 : 0.0;
    return SBLAS_OK;
}

}  // extern "C"

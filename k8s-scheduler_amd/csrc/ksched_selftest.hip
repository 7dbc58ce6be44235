// ksched_selftest.hip -- the device primitives run in isolation (diagnostics; no scheduling call launches these).
// Each kernel CALLS the inline functions of ksched_device.h, ksched_merge.h, ksched_pipe.h and ksched_commit.h on arrays of
// operands and stores what they return; no primitive's arithmetic is restated here.  Compiled with the library's
// flags, so the results are the source semantics of the primitives under those flags (-ffp-contract=off, ...), not
// the instruction stream of the kernels that inline them.  Element-wise kernels, or one wave per case; every loop
// bound is a launch argument.  tests/test_gpu_primitives.py compares the outputs with tests/screen_ref.py and the
// oracle's score.  At the end of the file, one level up: the stream pipeline's list-consuming stages (rank merge,
// both commits) launched alone on hand-built lists (ksched_selftest_rank_merge, ksched_selftest_commit).
#include <hip/hip_runtime.h>

#include <cstring>

#include "ksched_commit.h"
#include "ksched_ctx.h"
#include "ksched_merge.h"
#include "ksched_stream.h"

namespace ksched {

namespace {

// one element's operands: requests and allocatables (SoA: [3][n] each), their f64 forms and the hoisted reciprocals
// exactly as the kernels feed them (af = (double)a, y = recip_or_zero(a, af), y3 = recip(3.0))
struct PairOps {
    int64_t r[3], a[3];
    double rf[3], af[3], y[3], y3;
};
__device__ __forceinline__ PairOps load_ops(int64_t n, int64_t i, const int64_t *req, const int64_t *alloc) {
    PairOps o;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o.r[k] = req[k * n + i];
        o.a[k] = alloc[k * n + i];
        o.rf[k] = (double)o.r[k];
        o.af[k] = (double)o.a[k];
        o.y[k] = recip_or_zero(o.a[k], o.af[k]);
    }
    o.y3 = recip(3.0);
    return o;
}

}  // namespace

// score [3][n]: resource_score, resource_score_fast<false>, <true>; upper [2][n]: resource_score_upper<false>, <true>;
// rcp [3][n]: recip(af_k); flags: bit 0 / 1 near1 of upper<false> / <true>, bit 2 / 3 pair_key<resource>'s
// eligibility in the all-node / feasible domain, bit 4 fits()
__global__ void k_selftest_score(int64_t n, const int64_t *req, const int64_t *alloc, double *score, double *upper,
                                 double *rcp, int32_t *flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PairOps o = load_ops(n, i, req, alloc);
    score[i] = resource_score(o.r[0], o.r[1], o.r[2], o.rf[0], o.rf[1], o.rf[2], o.a[0], o.a[1], o.a[2], o.af[0],
                              o.af[1], o.af[2]);
    score[n + i] = resource_score_fast<false>(o.r[0], o.r[1], o.r[2], o.rf[0], o.rf[1], o.rf[2], o.a[0], o.a[1], o.a[2],
                                              o.af[0], o.af[1], o.af[2], o.y[0], o.y[1], o.y[2], o.y3);
    score[2 * n + i] = resource_score_fast<true>(o.r[0], o.r[1], o.r[2], o.rf[0], o.rf[1], o.rf[2], o.a[0], o.a[1],
                                                 o.a[2], o.af[0], o.af[1], o.af[2], o.y[0], o.y[1], o.y[2], o.y3);
    bool n0 = false, n1 = false;
    upper[i] = resource_score_upper<false>(o.r[0], o.r[1], o.r[2], o.rf[0], o.rf[1], o.rf[2], o.a[0], o.a[1], o.a[2],
                                           o.af[0], o.af[1], o.af[2], o.y[0], o.y[1], o.y[2], o.y3, &n0);
    upper[n + i] = resource_score_upper<true>(o.r[0], o.r[1], o.r[2], o.rf[0], o.rf[1], o.rf[2], o.a[0], o.a[1], o.a[2],
                                              o.af[0], o.af[1], o.af[2], o.y[0], o.y[1], o.y[2], o.y3, &n1);
#pragma unroll
    for (int k = 0; k < 3; ++k) rcp[k * n + i] = recip(o.af[k]);
    const bool feas = fits(o.r[0], o.r[1], o.r[2], 0ull, o.a[0], o.a[1], o.a[2], 0ull, false);
    double key;
    const bool ea = pair_key<kPrioResource, kDomAll>(feas, o.r[0], o.r[1], o.r[2], o.rf[0], o.rf[1], o.rf[2], o.a[0],
                                                     o.a[1], o.a[2], o.af[0], o.af[1], o.af[2], 0.0f, &key);
    const bool ef = pair_key<kPrioResource, kDomFeasible>(feas, o.r[0], o.r[1], o.r[2], o.rf[0], o.rf[1], o.rf[2],
                                                          o.a[0], o.a[1], o.a[2], o.af[0], o.af[1], o.af[2], 0.0f, &key);
    flags[i] = (n0 ? 1 : 0) | (n1 ? 2 : 0) | (ea ? 4 : 0) | (ef ? 8 : 0) | (feas ? 16 : 0);
}

__global__ void k_selftest_price(int64_t n, const float *price, double *key) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    key[i] = price_key(price[i]);
}

// The record pass 1 stores for one pair (ksched_pipe.hip, the keep_h loop): base by rf, 0 when ambiguous, 0xffff
// without a key; el: the pair carries a key in the domain.  PK: through the packed round-toward-zero conversion
// pass 1 uses, else through screen_rec / screen_rec_nf.
template <bool PK>
__device__ __forceinline__ uint32_t pass1_record(const ScreenV &sv, bool el) {
    if (sv.amb) return 0u;
    if (!el) return 0xffffu;
    if constexpr (PK) {
        const float w = __builtin_fmaxf((sv.rf ? 10.0f : kNfBase) - sv.v, 0.0f);
        const uint32_t rec = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(w, w));
        return (rec & 0xffffu) | (sv.rf ? 0u : 0x8000u);
    } else {
        return sv.rf ? screen_rec(sv.v) : screen_rec_nf(sv.v);
    }
}

// f [13][n]: screen_req x3, screen_recip x3, screen_y x3, screen_pair from screen_recip, screen_pair from screen_y,
//            screen_fast's v, mx
// u [8][n]:  lo_ok of the two screen_pair, amb, rf, then the pass-1 record: all-node domain by screen_rec*, by
//            cvt_pkrtz, feasible domain by screen_rec*, by cvt_pkrtz
__global__ void k_selftest_screen(int64_t n, const int64_t *req, const int64_t *alloc, float *f, uint32_t *u) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PairOps o = load_ops(n, i, req, alloc);
    float q[3], ys[3], yy[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        q[k] = screen_req(o.r[k]);
        ys[k] = screen_recip(o.a[k]);
        yy[k] = screen_y(o.a[k], o.y[k]);
        f[k * n + i] = q[k];
        f[(3 + k) * n + i] = ys[k];
        f[(6 + k) * n + i] = yy[k];
    }
    const bool okc = o.a[0] >= o.r[0], okm = o.a[1] >= o.r[1], okp = o.a[2] >= o.r[2];
    bool lo_s = false, lo_y = false;
    f[9 * n + i] = screen_pair(q[0], q[1], q[2], ys[0], ys[1], ys[2], okc, okm, okp, &lo_s);
    f[10 * n + i] = screen_pair(q[0], q[1], q[2], yy[0], yy[1], yy[2], okc, okm, okp, &lo_y);
    const ScreenV sv = screen_fast(q[0] * ys[0], q[1] * ys[1], q[2] * ys[2]);
    f[11 * n + i] = sv.v;
    f[12 * n + i] = sv.mx;
    u[i] = lo_s ? 1u : 0u;
    u[n + i] = lo_y ? 1u : 0u;
    u[2 * n + i] = sv.amb ? 1u : 0u;
    u[3 * n + i] = sv.rf ? 1u : 0u;
    u[4 * n + i] = pass1_record<false>(sv, true);
    u[5 * n + i] = pass1_record<true>(sv, true);
    u[6 * n + i] = pass1_record<false>(sv, sv.rf);  // no labels: feasible <=> every resource fits
    u[7 * n + i] = pass1_record<true>(sv, sv.rf);
}

// out [4][n]: screen_rec_w(w), screen_rec_w(w2), the low and the high half of cvt_pkrtz(w, w2)
__global__ void k_selftest_rec_w(int64_t n, const float *w, const float *w2, uint32_t *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float a = w[i], b = w2[i];
    out[i] = screen_rec_w(a);
    out[n + i] = screen_rec_w(b);
    const uint32_t pk = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(a, b));
    out[2 * n + i] = pk & 0xffffu;
    out[3 * n + i] = pk >> 16;
}

// out [4][n]: screen_rec_threshold(L), screen_rec_threshold_nf(L), screen_rec_needed(rec, those two),
// screen_rec_needed(rec, -1, -1) (an inactive lane)
__global__ void k_selftest_threshold(int64_t n, const float *L, const uint32_t *rec, int32_t *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int tq = screen_rec_threshold(L[i]), tqn = screen_rec_threshold_nf(L[i]);
    out[i] = tq;
    out[n + i] = tqn;
    out[2 * n + i] = screen_rec_needed(rec[i], tq, tqn) ? 1 : 0;
    out[3 * n + i] = screen_rec_needed(rec[i], -1, -1) ? 1 : 0;
}

// The seeded scan's primitives.  flags: bit 0 amb, bit 1 el.  x [6][n]: six lower bounds per element, inserted one by
// one into a sorted top-4 list (bound_insert<4>).  out [5][n]: screen_need(v, amb, el, L), then the list.
__global__ void k_selftest_seed(int64_t n, const float *v, const float *L, const uint32_t *flags, const uint32_t *x,
                                uint32_t *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = screen_need(v[i], (flags[i] & 1u) != 0, (flags[i] & 2u) != 0, L[i]) ? 1u : 0u;
    uint32_t t[4] = {0u, 0u, 0u, 0u};
    for (int s = 0; s < 6; ++s) bound_insert<4>(t, x[s * n + i]);
#pragma unroll
    for (int q = 0; q < 4; ++q) out[(1 + q) * n + i] = t[q];
}

// The commit's touched-node column (ksched_commit.h), element = one (pod, column) pair: the column's constants as its
// staging lane computes them (touch_stage on the state's recip_or_zero), the pod's screen value and decision
// (touch_need), and the column itself (touch_column<resource, all-node>) over each wave of 64 consecutive elements.
// f [4][n]: the staged reciprocals x3, the value; u [2][n]: needed, some element of the wave needed; key [n]: the
// column's key (exact where the wave needed it, kSkipKey otherwise)
__global__ void k_selftest_touch_screen(int64_t n, const int64_t *req, const int64_t *alloc, const float *thr,
                                        const uint32_t *active, float *f, uint32_t *u, double *key) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < n;  // (every lane of a wave reaches touch_column's ballot)
    const PairOps o = load_ops(n, in ? i : 0, req, alloc);
    const TouchY ty = touch_stage(o.a[0], o.a[1], o.a[2], o.y[0], o.y[1], o.y[2]);
    const float q0 = screen_req(o.r[0]), q1 = screen_req(o.r[1]), q2 = screen_req(o.r[2]);
    const float th = in ? thr[i] : 0.0f;
    const bool act = in && active[i] != 0;
    float v;
    const bool need = touch_need(q0, q1, q2, th, ty, o.r[0], o.r[1], o.r[2], o.a[0], o.a[1], o.a[2], act, &v);
    const bool feas = fits(o.r[0], o.r[1], o.r[2], 0ull, o.a[0], o.a[1], o.a[2], 0ull, false);
    const double fy[6] = {o.af[0], o.af[1], o.af[2], o.y[0], o.y[1], o.y[2]};
    double k;
    const bool any = touch_column<kPrioResource, kDomAll, false>(q0, q1, q2, th, ty, act, feas, o.r[0], o.r[1], o.r[2],
                                                                 o.rf[0], o.rf[1], o.rf[2], o.a[0], o.a[1], o.a[2], fy, o.y3,
                                                                 0.0f, &k);
    if (!in) return;
    f[i] = ty.c; f[n + i] = ty.m; f[2 * n + i] = ty.p; f[3 * n + i] = v;
    u[i] = need ? 1u : 0u;
    u[n + i] = any ? 1u : 0u;
    key[i] = k;
}

// ---- the wave primitives: one 64-lane workgroup per case, lane = element ------------------------------------------
template <int RUN>
__device__ __forceinline__ void sort_case(const WaveTestArgs &A, int r, int64_t nl, int64_t i, int lane) {
    uint64_t c = A.scode[r * nl + i];
    int32_t x = A.sidx[r * nl + i];
    wave_sort_desc<RUN>(c, x, lane);
    A.ocode[r * nl + i] = c;
    A.oidx[r * nl + i] = x;
}

__global__ __launch_bounds__(64) void k_selftest_wave(WaveTestArgs A) {
    const int64_t cs = blockIdx.x;
    if (cs >= A.ncases || threadIdx.x >= 64) return;  // uniform over the wave
    const int lane = (int)threadIdx.x;
    const int64_t nl = A.ncases * 64, i = cs * 64 + lane;
    sort_case<1>(A, 0, nl, i, lane);
    sort_case<2>(A, 1, nl, i, lane);
    sort_case<4>(A, 2, nl, i, lane);
    sort_case<8>(A, 3, nl, i, lane);
    sort_case<16>(A, 4, nl, i, lane);
    sort_case<32>(A, 5, nl, i, lane);
    // arrangement 0 again: each lane's rank among the 64 pairs, and the integer reductions
    const uint64_t c0 = A.scode[i];
    const int32_t x0 = A.sidx[i];
    A.rank[i] = wave_rank(c0, x0, c0, x0);
    A.red_max[i] = wave_max_u64(c0);
    A.red_sum[i] = wave_sum_i64((int64_t)c0);
    A.red_min[i] = wave_min_i32(x0);
    A.red_or[i] = wave_or_u64(c0);
    // the arg-bests of (key, idx) carrying aux
    const double k = A.key[i];
    const int32_t ki = A.kidx[i], ka = A.aux[i];
    {
        double bk = k;
        int32_t bi = ki, ba = ka;
        wave_argbest(bk, bi, ba);
        A.ab_key[i] = (uint64_t)__double_as_longlong(bk); A.ab_idx[i] = bi; A.ab_aux[i] = ba;
    }
    {
        double bk = k;
        int32_t bi = ki, ba = ka;
        wave_argbest_fast(bk, bi, ba);
        A.ab_key[nl + i] = (uint64_t)__double_as_longlong(bk); A.ab_idx[nl + i] = bi; A.ab_aux[nl + i] = ba;
    }
    const uint64_t kc = key_code(k);
    A.kcode[i] = kc;
    // a merged list's threshold: lanes < nv hold its valid entries
    A.thr[i] = list_thr_bits(A.cut[cs] != 0, __ballot(lane < A.nv[cs]), kc);
}

// lane = one sequence of S (key, idx) entries ([S][n]; idx kNoIdx: not inserted) into lists of KC = 2, 4, 8, 16
// ((-inf, kNoIdx) when empty, as every kernel starts them); okey / oidx [30][n]: the four lists one after the other
template <int KC>
__device__ __forceinline__ void list_case(int64_t n, int64_t i, int S, const double *key, const int32_t *idx, int row0,
                                          double *okey, int32_t *oidx) {
    double k[KC];
    int32_t x[KC];
#pragma unroll
    for (int q = 0; q < KC; ++q) { k[q] = -__builtin_inf(); x[q] = kNoIdx; }
    for (int j = 0; j < S; ++j) {
        const int32_t ci = idx[(int64_t)j * n + i];
        if (ci != kNoIdx) list_insert_ordered<KC>(k, x, key[(int64_t)j * n + i], ci);
    }
#pragma unroll
    for (int q = 0; q < KC; ++q) { okey[(int64_t)(row0 + q) * n + i] = k[q]; oidx[(int64_t)(row0 + q) * n + i] = x[q]; }
}

__global__ void k_selftest_list(int64_t n, int S, const double *key, const int32_t *idx, double *okey, int32_t *oidx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    list_case<2>(n, i, S, key, idx, 0, okey, oidx);
    list_case<4>(n, i, S, key, idx, 2, okey, oidx);
    list_case<8>(n, i, S, key, idx, 6, okey, oidx);
    list_case<16>(n, i, S, key, idx, 14, okey, oidx);
}

// The score role's slot helpers (ksched_pipe.h), per element: two sets of `steps` steps of kSlotRows lower bounds
// (x [2][steps][kSlotRows][n]) go through bound_slots<KC> into KC slots each, both sets are sorted (sort_desc_u32)
// and the second merged into the first (topk_merge_u32).  out rows from row0: the raw slots of set 0, of set 1, the
// sorted slots of set 0, of set 1, the merged list (KC rows each).  KC = 4 takes bound_slots' maximum form, KC = 8 its
// insertion form, as in k_pipe (4 rows per step of the screened scan).
constexpr int kSlotRows = 4;
template <int KC>
__device__ __forceinline__ void slots_case(int64_t n, int64_t i, int steps, const uint32_t *x, int row0, uint32_t *out) {
    uint32_t t[2][KC];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int q = 0; q < KC; ++q) t[h][q] = 0u;
        for (int j = 0; j < steps; ++j) {
            uint32_t xs[kSlotRows];
#pragma unroll
            for (int u = 0; u < kSlotRows; ++u) xs[u] = x[(((int64_t)h * steps + j) * kSlotRows + u) * n + i];
            bound_slots<KC>(t[h], xs);
        }
#pragma unroll
        for (int q = 0; q < KC; ++q) out[(int64_t)(row0 + h * KC + q) * n + i] = t[h][q];
        sort_desc_u32<KC>(t[h]);
#pragma unroll
        for (int q = 0; q < KC; ++q) out[(int64_t)(row0 + (2 + h) * KC + q) * n + i] = t[h][q];
    }
    topk_merge_u32<KC>(t[0], t[1]);
#pragma unroll
    for (int q = 0; q < KC; ++q) out[(int64_t)(row0 + 4 * KC + q) * n + i] = t[0][q];
}

// out [60][n]: slots_case<4> (20 rows), then slots_case<8> (40 rows)
__global__ void k_selftest_slots(int64_t n, int steps, const uint32_t *x, uint32_t *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    slots_case<4>(n, i, steps, x, 0, out);
    slots_case<8>(n, i, steps, x, 20, out);
}

// ------------------------------------------------------------------------------------------------
// launchers (device pointers; n > 0 elements or cases)
// ------------------------------------------------------------------------------------------------
namespace {
dim3 grid_of(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }
}  // namespace

hipError_t launch_selftest_score(int64_t n, const int64_t *req, const int64_t *alloc, double *score, double *upper,
                                 double *rcp, int32_t *flags, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_selftest_score, grid_of(n), dim3(256), 0, s, n, req, alloc, score, upper, rcp, flags);
    return hipGetLastError();
}

hipError_t launch_selftest_price(int64_t n, const float *price, double *key, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_selftest_price, grid_of(n), dim3(256), 0, s, n, price, key);
    return hipGetLastError();
}

hipError_t launch_selftest_screen(int64_t n, const int64_t *req, const int64_t *alloc, float *f, uint32_t *u,
                                  hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_selftest_screen, grid_of(n), dim3(256), 0, s, n, req, alloc, f, u);
    return hipGetLastError();
}

hipError_t launch_selftest_touch_screen(int64_t n, const int64_t *req, const int64_t *alloc, const float *thr,
                                        const uint32_t *active, float *f, uint32_t *u, double *key, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_selftest_touch_screen, grid_of(n), dim3(256), 0, s, n, req, alloc, thr, active, f, u, key);
    return hipGetLastError();
}

hipError_t launch_selftest_rec_w(int64_t n, const float *w, const float *w2, uint32_t *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_selftest_rec_w, grid_of(n), dim3(256), 0, s, n, w, w2, out);
    return hipGetLastError();
}

hipError_t launch_selftest_seed(int64_t n, const float *v, const float *L, const uint32_t *flags, const uint32_t *x,
                                uint32_t *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_selftest_seed, grid_of(n), dim3(256), 0, s, n, v, L, flags, x, out);
    return hipGetLastError();
}

hipError_t launch_selftest_threshold(int64_t n, const float *L, const uint32_t *rec, int32_t *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_selftest_threshold, grid_of(n), dim3(256), 0, s, n, L, rec, out);
    return hipGetLastError();
}

hipError_t launch_selftest_wave(const WaveTestArgs &a, hipStream_t s) {
    if (a.ncases <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_selftest_wave, dim3((unsigned)a.ncases), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_selftest_list(int64_t n, int S, const double *key, const int32_t *idx, double *okey, int32_t *oidx,
                                hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_selftest_list, grid_of(n), dim3(256), 0, s, n, S, key, idx, okey, oidx);
    return hipGetLastError();
}

hipError_t launch_selftest_slots(int64_t n, int steps, const uint32_t *x, uint32_t *out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_selftest_slots, grid_of(n), dim3(256), 0, s, n, steps, x, out);
    return hipGetLastError();
}

}  // namespace ksched

// ------------------------------------------------------------------------------------------------
// The list-consuming stages alone: the stream pipeline's rank merge and its two commits, each as ONE launch of the
// engine's own launcher (launch_rank_merge, launch_commit, launch_commit_spc; the control block by launch_ctl_init)
// on lists the caller built.  No kernel is restated or instantiated here.  Copy in, launch on c->stream, copy out,
// as the primitive self-tests do (ksched_data.hip).  tests/test_gpu_commit_alone.py compares with tests/commit_ref.py.
// ------------------------------------------------------------------------------------------------
using namespace ksched;

namespace {

// one device block of 256-byte aligned parts, freed with the object
struct StageBlock {
    char *d = nullptr;
    size_t total = 0;
    size_t take(size_t bytes) { const size_t o = total; total += (bytes + 255) / 256 * 256; return o; }
    hipError_t alloc() { return hipMalloc((void **)&d, total ? total : 256); }
    template <class T> T *at(size_t off) const { return reinterpret_cast<T *>(d + off); }
    ~StageBlock() { if (d) hipFree(d); }
};

// k_commit's admitted LDS, checked for either kernel as enqueue_batched checks it.  With B <= 128 and K <= 16 (at most
// 150528 bytes) it cannot trip: it stands for the day one of those limits moves.
constexpr size_t kStageSeqCommitMaxLds = 160 * 1024 - 4096;
constexpr int kStageSentinel = 0xa5;                         // every byte of a result nobody wrote

int stage_fail(ksched_ctx *c, const char *what, hipError_t e) {
    (void)hipGetLastError();
    return fail(c, KSCHED_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace

extern "C" {

int ksched_selftest_rank_merge(ksched_ctx *c, int32_t K, int32_t R, int32_t nb, const void *blocks, void *out_rec,
                               int64_t *out_fc) {
    if (!c) return KSCHED_E_INVALID;
    if ((K != 4 && K != 8 && K != 16) || R < 1 || R > 64 || nb < 1 || nb > 1024 || !blocks || !out_rec || !out_fc)
        return fail(c, KSCHED_E_INVALID, "selftest_rank_merge: K in {4, 8, 16}, 1 <= R <= 64, 1 <= nb <= 1024");
    HIPCHK(c, hipSetDevice(c->dev));
    const size_t rec_bytes = (size_t)nb * K * sizeof(Rec), fc_bytes = (size_t)nb * sizeof(int64_t);
    const size_t stride = rec_bytes + fc_bytes;
    StageBlock blk;
    const size_t o_in = blk.take(stride * R), o_cur = blk.take(8), o_rec = blk.take(rec_bytes), o_fc = blk.take(fc_bytes);
    HIPCHK(c, blk.alloc());
    hipStream_t s = c->stream;
    hipError_t e = hipMemcpyAsync(blk.d + o_in, blocks, stride * R, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(blk.d + o_cur, 0, 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(blk.d + o_rec, kStageSentinel, rec_bytes, s);
    if (e == hipSuccess) e = hipMemsetAsync(blk.d + o_fc, kStageSentinel, fc_bytes, s);
    if (e == hipSuccess) {
        MergeArgs mr{};
        mr.in = blk.d + o_in; mr.rank_stride = (int64_t)stride; mr.C_in = R; mr.C_out = 1;
        mr.cursor = blk.at<int64_t>(o_cur); mr.P = nb; mr.B = nb;
        mr.out_rec = blk.at<Rec>(o_rec); mr.out_fc = blk.at<int64_t>(o_fc);
        e = launch_rank_merge(K, mr, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(out_rec, blk.d + o_rec, rec_bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_fc, blk.d + o_fc, fc_bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return stage_fail(c, "selftest_rank_merge", e);
    return KSCHED_OK;
}

int ksched_selftest_commit(ksched_ctx *c, int32_t impl, int32_t K, int32_t B, int32_t prio, int32_t dom, int32_t lab,
                           int32_t f53, int32_t nb, const int64_t *rc, const int64_t *rm, const int64_t *rp,
                           const uint64_t *sel, const void *lists, const int64_t *fc0, const void *xin,
                           int32_t *out_idx, double *out_score, int32_t *out_feas, void *out_x, int64_t *out_ctl) {
    if (!c) return KSCHED_E_INVALID;
    if (!rc || !rm || !rp || !lists || !fc0 || !xin || !out_idx || !out_score || !out_feas || !out_x || !out_ctl)
        return fail(c, KSCHED_E_INVALID, "selftest_commit: null argument");
    const bool spc = impl == KSCHED_COMMIT_SPECULATIVE;
    if (!spc && impl != KSCHED_COMMIT_SEQUENTIAL) return fail(c, KSCHED_E_INVALID, "selftest_commit: impl");
    if ((K != 4 && K != 8 && K != 16) || B < 1 || B > 128 || nb < 1 || nb > B || (spc && B > 64) ||
        (prio != kPrioResource && prio != kPrioPrice) || (dom != kDomAll && dom != kDomFeasible))
        return fail(c, KSCHED_E_INVALID, "selftest_commit: K in {4, 8, 16}, 1 <= nb <= batch <= 128 (speculative: 64)");
    if (commit_lds_bytes(B, K) > kStageSeqCommitMaxLds)
        return fail(c, KSCHED_E_INVALID, "selftest_commit: B*(328+48K) <= ~150 KB of LDS");
    int32_t nin = 0;
    memcpy(&nin, xin, sizeof(nin));  // XBuf::count
    if (nin < 0 || nin > (spc ? 64 : B))
        return fail(c, KSCHED_E_INVALID, "selftest_commit: inherited export over 64 (speculative) or the batch (sequential)");
    HIPCHK(c, hipSetDevice(c->dev));
    const size_t q = (size_t)nb, xb = xbuf_bytes(B), list_bytes = q * K * sizeof(Rec);
    // the inherited export may hold 64 records whatever B (speculative kernel): its part is sized for the larger of
    // the engine's buffer (2 B records) and 64 records.  A batch exports at most one record per pod (<= B).
    const size_t xin_room = std::max(xb, 16 + (size_t)64 * sizeof(XRec));
    StageBlock blk;
    const size_t o_rc = blk.take(q * 8), o_rm = blk.take(q * 8), o_rp = blk.take(q * 8), o_sel = blk.take(q * 8);
    const size_t o_lists = blk.take(list_bytes), o_fc0 = blk.take(q * 8), o_xin = blk.take(xin_room), o_xout = blk.take(xb);
    const size_t o_idx = blk.take(q * 4), o_sc = blk.take(q * 8), o_feas = blk.take(q * 4), o_ctl = blk.take(sizeof(Ctl));
    HIPCHK(c, blk.alloc());
    hipStream_t s = c->stream;
    const size_t xin_bytes = 16 + (size_t)nin * sizeof(XRec);
    if (xin_bytes > xin_room) return fail(c, KSCHED_E_INVALID, "selftest_commit: inherited export over its buffer");
    hipError_t e = hipMemcpyAsync(blk.d + o_rc, rc, q * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(blk.d + o_rm, rm, q * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(blk.d + o_rp, rp, q * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = sel ? hipMemcpyAsync(blk.d + o_sel, sel, q * 8, hipMemcpyHostToDevice, s) : hipMemsetAsync(blk.d + o_sel, 0, q * 8, s);
    if (e == hipSuccess) e = hipMemcpyAsync(blk.d + o_lists, lists, list_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(blk.d + o_fc0, fc0, q * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(blk.d + o_xin, 0, xin_room, s);
    if (e == hipSuccess) e = hipMemcpyAsync(blk.d + o_xin, xin, xin_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(blk.d + o_xout, kStageSentinel, xb, s);
    if (e == hipSuccess) e = hipMemsetAsync(blk.d + o_idx, kStageSentinel, q * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(blk.d + o_sc, kStageSentinel, q * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(blk.d + o_feas, kStageSentinel, q * 4, s);
    Ctl *ctl = blk.at<Ctl>(o_ctl);
    if (e == hipSuccess) e = hipMemsetAsync(ctl, 0, sizeof(Ctl), s);
    if (e == hipSuccess) e = launch_ctl_init(ctl, B, nb, 2, s);  // as enqueue_batched: plan[0] = 0, plan[1] = -1 (nb <= B)
    if (e == hipSuccess) {
        CommitArgs ca{};  // every persistent-pipeline field stays null / zero
        ca.lists = blk.at<Rec>(o_lists); ca.fc0 = blk.at<int64_t>(o_fc0);
        ca.pods = PodArgs{blk.at<int64_t>(o_rc), blk.at<int64_t>(o_rm), blk.at<int64_t>(o_rp), blk.at<uint64_t>(o_sel), nb};
        ca.plan = &ctl->plan[0]; ca.plan1 = &ctl->plan[1]; ca.plan2 = &ctl->plan[2];
        ca.ctl = ctl; ca.B = B;
        ca.xin = blk.at<XBuf>(o_xin); ca.xout = blk.at<XBuf>(o_xout);
        ca.out = OutArgs{blk.at<int32_t>(o_idx), blk.at<double>(o_sc), blk.at<int32_t>(o_feas)};
        ca.batch = 0;
        e = spc ? launch_commit_spc(K, prio, dom, lab != 0, f53 != 0, ca, s)
                : launch_commit(K, prio, dom, lab != 0, f53 != 0, ca, commit_lds_bytes(B, K), s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    Ctl h{};
    if (e == hipSuccess) e = hipMemcpy(&h, ctl, sizeof(Ctl), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_idx, blk.d + o_idx, q * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_score, blk.d + o_sc, q * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_feas, blk.d + o_feas, q * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_x, blk.d + o_xout, xb, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return stage_fail(c, "selftest_commit", e);
    out_ctl[0] = h.cursor; out_ctl[1] = h.stats[0]; out_ctl[2] = h.stats[1]; out_ctl[3] = h.stats[2]; out_ctl[4] = h.plan[2];
    return KSCHED_OK;
}

}  // extern "C"

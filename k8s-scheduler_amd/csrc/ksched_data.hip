// ksched_data.hip -- libksched: the calls that move data in and out of a context.  Node rows (load, delta, read,
// save / restore), pending pods, per-pod results, and the FailedScheduling explanations.
#include <cmath>
#include <cstring>

#include <new>

#include "ksched_ctx.h"
#include "ksched_preempt.h"
#include "ksched_preemptc.h"
#include "ksched_rank.h"

using namespace ksched;

static uint64_t uabs(int64_t v) { return v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v; }

// The bound-pod table, grouped and laid out for the device (ksched_preempt.h: BoundTable).  A counting sort by node
// keeps the table's order inside a node; reading a segment backwards and stable-sorting it by priority then gives
// ascending importance (prio ascending, table index descending).
bool ksched::build_bound_table(int64_t n, int64_t nb, const int32_t *node_idx, const int64_t *cpu, const int64_t *mem,
                               const int32_t *prio, BoundTableHost *out, const char **why) {
    const int64_t blocks = (n + 63) / 64;
    out->seg.assign((size_t)n, 0);
    for (int64_t t = 0; t < nb; ++t) {
        if (node_idx[t] < 0 || node_idx[t] >= n) { *why = "node index out of range"; return false; }
        if (++out->seg[(size_t)node_idx[t]] > kBoundMaxPerNode) { *why = "more than KSCHED_BOUND_MAX_PER_NODE pods on one node"; return false; }
    }
    std::vector<int64_t> start((size_t)n + 1, 0);  // the counting sort: node j's pods are order[start[j] .. start[j + 1])
    for (int64_t j = 0; j < n; ++j) start[(size_t)j + 1] = start[(size_t)j] + out->seg[(size_t)j];
    std::vector<int32_t> order((size_t)nb);
    {
        std::vector<int64_t> at(start.begin(), start.end() - 1);
        for (int64_t t = 0; t < nb; ++t) order[(size_t)at[(size_t)node_idx[t]]++] = (int32_t)t;
    }
    out->off.assign((size_t)blocks, 0);
    out->depth.assign((size_t)blocks, 0);
    int64_t entries = 0;
    for (int64_t b = 0; b < blocks; ++b) {
        int32_t d = 0;
        for (int64_t j = b * 64; j < std::min<int64_t>(n, b * 64 + 64); ++j) d = std::max(d, out->seg[(size_t)j]);
        out->off[(size_t)b] = entries;
        out->depth[(size_t)b] = d;
        entries += (int64_t)d * 64;
    }
    out->cpu.assign((size_t)entries, 0);
    out->mem.assign((size_t)entries, 0);
    out->prio.assign((size_t)entries, INT32_MAX);  // padding: below no preemptor's priority
    out->tidx.assign((size_t)entries, -1);
    for (int64_t j = 0; j < n; ++j) {
        int32_t *lo = order.data() + start[(size_t)j], *hi = order.data() + start[(size_t)j + 1];
        std::reverse(lo, hi);  // table index descending ...
        std::stable_sort(lo, hi, [&](int32_t x, int32_t y) { return prio[x] < prio[y]; });  // ... within a priority
        const int64_t e0 = out->off[(size_t)(j >> 6)] + (j & 63);
        for (int32_t *q = lo; q < hi; ++q) {
            const size_t e = (size_t)(e0 + (int64_t)(q - lo) * 64);
            out->cpu[e] = cpu[*q]; out->mem[e] = mem[*q]; out->prio[e] = prio[*q]; out->tidx[e] = *q;
        }
    }
    return true;
}

// The primitive self-tests (ksched_selftest.hip), all in ksched_selftest_fastdiv's pattern: copy in, launch on c->stream, copy out.
// One device block holds every array (256-byte aligned); launch(in, out) gets their device pointers in order.
namespace {
struct StBuf {
    const void *in;  // host source (inputs), or nullptr
    void *out;       // host destination (outputs), or nullptr
    size_t bytes;
};
template <typename Launch>
int selftest_run(ksched_ctx *c, const char *what, const std::vector<StBuf> &bufs, Launch launch) {
    for (const StBuf &b : bufs)
        if (b.bytes > 0 && !b.in && !b.out) return KSCHED_E_INVALID;
    HIPCHK(c, hipSetDevice(c->dev));
    std::vector<size_t> off(bufs.size());
    size_t total = 0;
    for (size_t k = 0; k < bufs.size(); ++k) { off[k] = total; total += (bufs[k].bytes + 255) / 256 * 256; }
    char *d = nullptr;
    HIPCHK(c, hipMalloc(&d, total ? total : 256));
    std::vector<void *> p(bufs.size());
    for (size_t k = 0; k < bufs.size(); ++k) p[k] = d + off[k];
    hipError_t e = hipSuccess;
    for (size_t k = 0; k < bufs.size() && e == hipSuccess; ++k)
        if (bufs[k].in && bufs[k].bytes) e = hipMemcpyAsync(p[k], bufs[k].in, bufs[k].bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch(p);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    for (size_t k = 0; k < bufs.size() && e == hipSuccess; ++k)
        if (bufs[k].out && bufs[k].bytes) e = hipMemcpy(bufs[k].out, p[k], bufs[k].bytes, hipMemcpyDeviceToHost);
    hipFree(d);
    if (e != hipSuccess) return fail(c, KSCHED_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return KSCHED_OK;
}
}  // namespace

extern "C" {

int ksched_load_nodes(ksched_ctx *c, int64_t n, const int64_t *ac, const int64_t *am, const int64_t *ap,
                      const uint64_t *labels, const float *price) {
    if (!c) return KSCHED_E_INVALID;
    if (n < 0 || (n > 0 && (!ac || !am || !ap))) return fail(c, KSCHED_E_INVALID, "load_nodes: bad arguments");
    if (c->o.use_labels && n > 0 && !labels) return fail(c, KSCHED_E_INVALID, "load_nodes: use_labels needs labels");
    if (c->o.priority == KSCHED_PRIORITY_BEST_PRICE && n > 0 && !price)
        return fail(c, KSCHED_E_INVALID, "load_nodes: best-price priority needs prices");
    // node indices are int32 on the device and kNoIdx (INT32_MAX) marks "no candidate": every global
    // index this rank produces (node_offset + local) must stay below it
    if (c->o.node_offset < 0 || n > 0x7ffffff0LL || c->o.node_offset + n > 0x7ffffff0LL)
        return fail(c, KSCHED_E_INVALID, "load_nodes: node_offset + n must stay below 2^31 - 16");
    std::vector<NodeRec> h((size_t)std::max<int64_t>(n, 0));
    uint64_t mx = 0;
    for (int64_t i = 0; i < n; ++i) {
        NodeRec &r = h[(size_t)i];
        r.a[0] = ac[i]; r.a[1] = am[i]; r.a[2] = ap[i];
        r.af[0] = r.af[1] = r.af[2] = 0.0;  // derived on the device (k_prep_nodes) with the reciprocals
        r.y[0] = r.y[1] = r.y[2] = 0.0;
        r.labels = labels ? labels[i] : 0;
        r.price = (price && price[i] != 0.f) ? price[i] : 0.f;  // "-0" == "0": canonical +0 (price_key)
        r.ys[0] = r.ys[1] = r.ys[2] = 0.f;
        mx = std::max(mx, std::max(uabs(ac[i]), std::max(uabs(am[i]), uabs(ap[i]))));
        if (price && !std::isfinite(price[i])) return fail(c, KSCHED_E_INVALID, "load_nodes: non-finite price");
    }
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->perm_n = -1;  // first: whatever happens below, d->perm no longer describes the loaded nodes
    c->bound_valid = false;  // ... and neither does the bound-pod table (ksched_load_bound)
    c->spread_D = c->spread_S = 0;  // ... nor the spread table (ksched_load_spread)
    c->ext_R = 0;  // ... nor the extended-resource table (ksched_load_ext)
    c->aff_valid = false;  // ... nor the affinity table (ksched_load_affinity)
    HIPCHK(c, c->d->nodes.reserve((size_t)n * sizeof(NodeRec)));
    c->d->snap.release();
    // in the stream of the kernels that read it (a legacy hipMemcpy from pageable memory may return before its DMA
    // lands, and nothing orders it with this non-blocking stream: k_prep_nodes read the memory's earlier contents --
    // the round-4 exchange failure)
    if (n > 0) HIPCHK(c, hipMemcpyAsync(c->d->nodes, h.data(), (size_t)n * sizeof(NodeRec), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_prep_nodes(c->d->nodes, n, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->max_abs_alloc = mx;
    c->n_local = n;
    c->explain_valid = false;
    c->n_global = c->o.nranks > 1 ? c->o.nodes_global : (c->o.nodes_global > 0 ? c->o.nodes_global : n);
    if (c->n_global < c->o.node_offset + n) return fail(c, KSCHED_E_INVALID, "load_nodes: nodes_global too small");
    if (price && n > 0 && n <= (int64_t)kExact1Block * 16) {
        // exact mode on one workgroup (k_exact1): the nodes in the best-price argmax's order -- price ascending,
        // node index ascending on ties (prices are finite, -0 canonical: the order of price_key descending)
        std::vector<int32_t> perm((size_t)n);
        for (int64_t i = 0; i < n; ++i) perm[(size_t)i] = (int32_t)i;
        std::stable_sort(perm.begin(), perm.end(), [&](int32_t x, int32_t y) { return h[(size_t)x].price < h[(size_t)y].price; });
        HIPCHK(c, c->d->perm.reserve((size_t)n * sizeof(int32_t)));
        HIPCHK(c, hipMemcpyAsync(c->d->perm, perm.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->perm_n = n;
    } else {
        c->d->perm.release();
    }
    return KSCHED_OK;
}

int ksched_apply_delta(ksched_ctx *c, int64_t k, const int32_t *idx, const int64_t *dc, const int64_t *dm,
                       const int64_t *dp) {
    if (!c) return KSCHED_E_INVALID;
    if (c->n_local < 0) return fail(c, KSCHED_E_STATE, "apply_delta before load_nodes");
    if (k < 0 || (k > 0 && (!idx || !dc || !dm || !dp))) return fail(c, KSCHED_E_INVALID, "apply_delta: bad arguments");
    if (k == 0) return KSCHED_OK;
    for (int64_t i = 0; i < k; ++i) {
        if (idx[i] < 0 || idx[i] >= c->n_local) return fail(c, KSCHED_E_INVALID, "apply_delta: node index out of range");
        c->max_abs_alloc = sat_add(c->max_abs_alloc, sat_add(uabs(dc[i]), sat_add(uabs(dm[i]), uabs(dp[i]))));
    }
    HIPCHK(c, hipSetDevice(c->dev));
    std::vector<int64_t> d((size_t)(3 * k));
    std::memcpy(d.data(), dc, (size_t)k * 8);
    std::memcpy(d.data() + k, dm, (size_t)k * 8);
    std::memcpy(d.data() + 2 * k, dp, (size_t)k * 8);
    int32_t *d_idx = nullptr;
    int64_t *d_d = nullptr;
    HIPCHK(c, hipMalloc(&d_idx, (size_t)k * 4));
    if (hipMalloc(&d_d, (size_t)k * 24) != hipSuccess) { hipFree(d_idx); return fail(c, KSCHED_E_DEVICE, "apply_delta: alloc"); }
    hipError_t e = hipMemcpyAsync(d_idx, idx, (size_t)k * 4, hipMemcpyHostToDevice, c->stream);  // the kernel's stream
    if (e == hipSuccess) e = hipMemcpyAsync(d_d, d.data(), (size_t)k * 24, hipMemcpyHostToDevice, c->stream);
    c->explain_valid = false;
    if (e == hipSuccess) e = launch_apply_delta(c->d->nodes, c->n_local, k, d_idx, d_d, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(d_idx);
    hipFree(d_d);
    if (e != hipSuccess) return fail(c, KSCHED_E_DEVICE, std::string("apply_delta: ") + hipGetErrorString(e));
    return KSCHED_OK;
}

int ksched_explain(ksched_ctx *c, int64_t rc, int64_t rm, int64_t rp, uint64_t sel, int64_t out_counts[KSCHED_NUM_REASONS],
                   uint8_t *out_reason) {
    if (!c) return KSCHED_E_INVALID;
    if (c->n_local < 0) return fail(c, KSCHED_E_STATE, "explain before load_nodes");
    if (!out_counts) return fail(c, KSCHED_E_INVALID, "explain: out_counts is NULL");
    static_assert(KSCHED_NUM_REASONS == kNumReasons, "reason codes");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t n = c->n_local;
    unsigned long long *d_cnt = nullptr;
    HIPCHK(c, hipMalloc(&d_cnt, KSCHED_NUM_REASONS * sizeof(unsigned long long) + (size_t)(out_reason ? n : 0)));
    uint8_t *d_reason = out_reason ? (uint8_t *)(d_cnt + KSCHED_NUM_REASONS) : nullptr;
    unsigned long long h[KSCHED_NUM_REASONS] = {};
    hipError_t e = hipMemsetAsync(d_cnt, 0, KSCHED_NUM_REASONS * sizeof(unsigned long long), c->stream);
    if (e == hipSuccess)
        e = launch_explain(c->d->nodes, n, rc, rm, rp, sel, c->o.use_labels != 0, d_reason, d_cnt, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(h, d_cnt, sizeof(h), hipMemcpyDeviceToHost);
    if (e == hipSuccess && out_reason && n > 0) e = hipMemcpy(out_reason, d_reason, (size_t)n, hipMemcpyDeviceToHost);
    hipFree(d_cnt);
    if (e != hipSuccess) return fail(c, KSCHED_E_DEVICE, std::string("explain: ") + hipGetErrorString(e));
    for (int k = 0; k < KSCHED_NUM_REASONS; ++k) out_counts[k] = (int64_t)h[k];
    return KSCHED_OK;
}

static ExplainArgs explain_args(ksched_ctx *c) {
    ExplainArgs a{};
    a.idx = c->d->oidx; a.p = c->p;
    a.rc = c->d->rc; a.rm = c->d->rm; a.rp = c->d->rp; a.sel = c->d->sel;
    a.nodes = c->d->nodes; a.n_local = c->n_local; a.node_lo = c->o.node_offset;
    a.use_labels = c->o.use_labels != 0;
    return a;
}

int ksched_explain_batch(ksched_ctx *c, int64_t p, int64_t *out_counts, int64_t *out_nofit) {
    if (!c) return KSCHED_E_INVALID;
    if (!out_counts && p > 0) return fail(c, KSCHED_E_INVALID, "explain_batch: out_counts is NULL");
    if (p != c->p) return fail(c, KSCHED_E_INVALID, "explain_batch: p differs from the last schedule call");
    if (!c->explain_valid) return fail(c, KSCHED_E_STATE, "explain_batch: the node state changed since the last schedule call");
    if (p >= 0x7fffffff) return fail(c, KSCHED_E_INVALID, "explain_batch: too many pods");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memset(out_counts, 0, (size_t)p * KSCHED_NUM_REASONS * sizeof(int64_t));
    if (out_nofit) *out_nofit = 0;
    if (p == 0 || c->n_local == 0) return KSCHED_OK;
    const size_t cnt_bytes = (size_t)p * kNumReasons * sizeof(unsigned long long);
    HIPCHK(c, c->d->xbuf.reserve(std::max<size_t>(256, cnt_bytes + (size_t)p * sizeof(int32_t))));
    unsigned long long *d_cnt = static_cast<unsigned long long *>(c->d->xbuf.p);
    int32_t *d_fpod = reinterpret_cast<int32_t *>(static_cast<char *>(c->d->xbuf.p) + cnt_bytes);
    HIPCHK(c, hipMemsetAsync(d_cnt, 0, cnt_bytes, c->stream));
    ExplainArgs a = explain_args(c);
    int64_t nf = 0;
    a.fpod_out = d_fpod;
    a.n_nofit = &nf;
    HIPCHK(c, explain_batch(a, &c->d->xws.p, &c->d->xws.bytes, d_cnt, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nf == 0) return KSCHED_OK;
    std::vector<unsigned long long> h((size_t)nf * kNumReasons);
    std::vector<int32_t> fp((size_t)nf);
    HIPCHK(c, hipMemcpy(h.data(), d_cnt, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(fp.data(), d_fpod, fp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int64_t f = 0; f < nf; ++f)
        for (int r = 0; r < kNumReasons; ++r)
            out_counts[(size_t)fp[(size_t)f] * kNumReasons + r] = (int64_t)h[(size_t)f * kNumReasons + r];
    if (out_nofit) *out_nofit = nf;
    return KSCHED_OK;
}

int ksched_explain_pod(ksched_ctx *c, int64_t pod, int64_t out_counts[KSCHED_NUM_REASONS], uint8_t *out_reason) {
    if (!c) return KSCHED_E_INVALID;
    if (!out_counts) return fail(c, KSCHED_E_INVALID, "explain_pod: out_counts is NULL");
    if (pod < 0 || pod >= c->p) return fail(c, KSCHED_E_INVALID, "explain_pod: pod out of range");
    if (!c->explain_valid) return fail(c, KSCHED_E_STATE, "explain_pod: the node state changed since the last schedule call");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t n = c->n_local;
    ExplainArgs a = explain_args(c);
    HIPCHK(c, hipMemcpy(&a.q_rc, c->d->rc + pod, 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&a.q_rm, c->d->rm + pod, 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&a.q_rp, c->d->rp + pod, 8, hipMemcpyDeviceToHost));
    if (c->o.use_labels) HIPCHK(c, hipMemcpy(&a.q_sel, c->d->sel + pod, 8, hipMemcpyDeviceToHost));
    const size_t st_bytes = (size_t)3 * std::max<int64_t>(n, 1) * sizeof(int64_t);
    HIPCHK(c, c->d->xbuf.reserve(std::max<size_t>(256, st_bytes + 64 + (size_t)std::max<int64_t>(n, 1))));
    int64_t *d_state = static_cast<int64_t *>(c->d->xbuf.p);
    unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(static_cast<char *>(c->d->xbuf.p) + st_bytes);
    uint8_t *d_reason = reinterpret_cast<uint8_t *>(d_cnt + 8);
    HIPCHK(c, hipMemsetAsync(d_cnt, 0, kNumReasons * sizeof(unsigned long long), c->stream));
    HIPCHK(c, explain_pod_at(a, pod, d_state, out_reason ? d_reason : nullptr, d_cnt, c->stream));
    unsigned long long h[kNumReasons] = {};
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h, d_cnt, sizeof(h), hipMemcpyDeviceToHost));
    if (out_reason && n > 0) HIPCHK(c, hipMemcpy(out_reason, d_reason, (size_t)n, hipMemcpyDeviceToHost));
    for (int r = 0; r < kNumReasons; ++r) out_counts[r] = (int64_t)h[r];
    return KSCHED_OK;
}

int ksched_read_nodes(ksched_ctx *c, int64_t n, int64_t *ac, int64_t *am, int64_t *ap) {
    if (!c) return KSCHED_E_INVALID;
    if (c->n_local < 0) return fail(c, KSCHED_E_STATE, "read_nodes before load_nodes");
    if (n != c->n_local) return fail(c, KSCHED_E_INVALID, "read_nodes: size mismatch");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<NodeRec> h((size_t)n);
    if (n > 0) HIPCHK(c, hipMemcpy(h.data(), c->d->nodes, (size_t)n * sizeof(NodeRec), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) {
        if (ac) ac[i] = h[(size_t)i].a[0];
        if (am) am[i] = h[(size_t)i].a[1];
        if (ap) ap[i] = h[(size_t)i].a[2];
    }
    return KSCHED_OK;
}

int ksched_save_state(ksched_ctx *c) {
    if (!c) return KSCHED_E_INVALID;
    if (c->n_local < 0) return fail(c, KSCHED_E_STATE, "save_state before load_nodes");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, c->d->snap.reserve((size_t)c->n_local * sizeof(NodeRec)));  // (released by every load_nodes)
    if (c->n_local > 0)
        HIPCHK(c, hipMemcpyAsync(c->d->snap, c->d->nodes, (size_t)c->n_local * sizeof(NodeRec), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->snap_max_abs_alloc = c->max_abs_alloc;
    return KSCHED_OK;
}

int ksched_restore_state(ksched_ctx *c) {
    if (!c) return KSCHED_E_INVALID;
    if (!c->d->snap) return fail(c, KSCHED_E_STATE, "restore_state without save_state");
    HIPCHK(c, hipSetDevice(c->dev));
    if (c->n_local > 0)
        HIPCHK(c, hipMemcpyAsync(c->d->nodes, c->d->snap, (size_t)c->n_local * sizeof(NodeRec), hipMemcpyDeviceToDevice, c->stream));
    c->max_abs_alloc = c->snap_max_abs_alloc;
    c->explain_valid = false;
    return KSCHED_OK;
}

int ksched_upload_pods(ksched_ctx *c, int64_t p, const int64_t *rc, const int64_t *rm, const int64_t *rp,
                       const uint64_t *sel) {
    if (!c) return KSCHED_E_INVALID;
    if (p < 0 || (p > 0 && (!rc || !rm || !rp))) return fail(c, KSCHED_E_INVALID, "upload_pods: bad arguments");
    if (c->o.use_labels && p > 0 && !sel) return fail(c, KSCHED_E_INVALID, "upload_pods: use_labels needs selectors");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t q = (size_t)p;
    HIPCHK(c, c->d->rc.reserve(q * 8)); HIPCHK(c, c->d->rm.reserve(q * 8));
    HIPCHK(c, c->d->rp.reserve(q * 8)); HIPCHK(c, c->d->sel.reserve(q * 8));
    HIPCHK(c, c->d->oidx.reserve(q * 4)); HIPCHK(c, c->d->osc.reserve(q * 8));
    HIPCHK(c, c->d->ofeas.reserve(q * 4));
    if (p > 0) {
        // in the stream of the kernels that read them, finished before the caller's buffers may change (see
        // ksched_load_nodes)
        HIPCHK(c, hipMemcpyAsync(c->d->rc, rc, (size_t)p * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d->rm, rm, (size_t)p * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d->rp, rp, (size_t)p * 8, hipMemcpyHostToDevice, c->stream));
        if (sel) HIPCHK(c, hipMemcpyAsync(c->d->sel, sel, (size_t)p * 8, hipMemcpyHostToDevice, c->stream));
        else HIPCHK(c, hipMemsetAsync(c->d->sel, 0, (size_t)p * 8, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    uint64_t sum = 0;
    for (int64_t i = 0; i < p; ++i) sum = sat_add(sum, sat_add(uabs(rc[i]), sat_add(uabs(rm[i]), uabs(rp[i]) + 1)));
    c->sum_abs_req = sum;
    c->p = p;
    c->explain_valid = false;
    return KSCHED_OK;
}

int ksched_selftest_fastdiv(ksched_ctx *c, int64_t n, const double *a, const double *b, double *out_native,
                            double *out_fast) {
    if (!c || n < 0 || (n > 0 && (!a || !b || !out_native || !out_fast))) return KSCHED_E_INVALID;
    if (n == 0) return KSCHED_OK;
    HIPCHK(c, hipSetDevice(c->dev));
    double *d = nullptr;
    HIPCHK(c, hipMalloc(&d, (size_t)n * 32));
    hipError_t e = hipMemcpyAsync(d, a, (size_t)n * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + n, b, (size_t)n * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_selftest_div(n, d, d + n, d + 2 * n, d + 3 * n, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out_native, d + 2 * n, (size_t)n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_fast, d + 3 * n, (size_t)n * 8, hipMemcpyDeviceToHost);
    hipFree(d);
    if (e != hipSuccess) return fail(c, KSCHED_E_DEVICE, std::string("selftest_fastdiv: ") + hipGetErrorString(e));
    return KSCHED_OK;
}

// The primitive self-tests (ksched_selftest.hip), all in the pattern above (selftest_run).
int ksched_selftest_score(ksched_ctx *c, int64_t n, const int64_t *req, const int64_t *alloc, double *out_score,
                          double *out_upper, double *out_recip, int32_t *out_flags) {
    if (!c || n < 0 || (n > 0 && (!req || !alloc || !out_score || !out_upper || !out_recip || !out_flags)))
        return KSCHED_E_INVALID;
    if (n == 0) return KSCHED_OK;
    const size_t q = (size_t)n;
    return selftest_run(c, "selftest_score",
                        {{req, nullptr, q * 24}, {alloc, nullptr, q * 24}, {nullptr, out_score, q * 24},
                         {nullptr, out_upper, q * 16}, {nullptr, out_recip, q * 24}, {nullptr, out_flags, q * 4}},
                        [&](const std::vector<void *> &p) {
                            return launch_selftest_score(n, (const int64_t *)p[0], (const int64_t *)p[1], (double *)p[2],
                                                         (double *)p[3], (double *)p[4], (int32_t *)p[5], c->stream);
                        });
}

int ksched_selftest_price_key(ksched_ctx *c, int64_t n, const float *price, double *out_key) {
    if (!c || n < 0 || (n > 0 && (!price || !out_key))) return KSCHED_E_INVALID;
    if (n == 0) return KSCHED_OK;
    const size_t q = (size_t)n;
    return selftest_run(c, "selftest_price_key", {{price, nullptr, q * 4}, {nullptr, out_key, q * 8}},
                        [&](const std::vector<void *> &p) {
                            return launch_selftest_price(n, (const float *)p[0], (double *)p[1], c->stream);
                        });
}

int ksched_selftest_screen(ksched_ctx *c, int64_t n, const int64_t *req, const int64_t *alloc, float *out_f32,
                           uint32_t *out_u32) {
    if (!c || n < 0 || (n > 0 && (!req || !alloc || !out_f32 || !out_u32))) return KSCHED_E_INVALID;
    if (n == 0) return KSCHED_OK;
    const size_t q = (size_t)n;
    return selftest_run(c, "selftest_screen",
                        {{req, nullptr, q * 24}, {alloc, nullptr, q * 24}, {nullptr, out_f32, q * 13 * 4},
                         {nullptr, out_u32, q * 8 * 4}},
                        [&](const std::vector<void *> &p) {
                            return launch_selftest_screen(n, (const int64_t *)p[0], (const int64_t *)p[1], (float *)p[2],
                                                          (uint32_t *)p[3], c->stream);
                        });
}

int ksched_selftest_rec_w(ksched_ctx *c, int64_t n, const float *w, const float *w2, uint32_t *out) {
    if (!c || n < 0 || (n > 0 && (!w || !w2 || !out))) return KSCHED_E_INVALID;
    if (n == 0) return KSCHED_OK;
    const size_t q = (size_t)n;
    return selftest_run(c, "selftest_rec_w", {{w, nullptr, q * 4}, {w2, nullptr, q * 4}, {nullptr, out, q * 16}},
                        [&](const std::vector<void *> &p) {
                            return launch_selftest_rec_w(n, (const float *)p[0], (const float *)p[1], (uint32_t *)p[2],
                                                         c->stream);
                        });
}

int ksched_selftest_threshold(ksched_ctx *c, int64_t n, const float *L, const uint32_t *rec, int32_t *out) {
    if (!c || n < 0 || (n > 0 && (!L || !rec || !out))) return KSCHED_E_INVALID;
    if (n == 0) return KSCHED_OK;
    const size_t q = (size_t)n;
    return selftest_run(c, "selftest_threshold", {{L, nullptr, q * 4}, {rec, nullptr, q * 4}, {nullptr, out, q * 16}},
                        [&](const std::vector<void *> &p) {
                            return launch_selftest_threshold(n, (const float *)p[0], (const uint32_t *)p[1],
                                                             (int32_t *)p[2], c->stream);
                        });
}

int ksched_selftest_seed(ksched_ctx *c, int64_t n, const float *v, const float *L, const uint32_t *flags,
                         const uint32_t *x, uint32_t *out) {
    if (!c || n < 0 || (n > 0 && (!v || !L || !flags || !x || !out))) return KSCHED_E_INVALID;
    if (n == 0) return KSCHED_OK;
    const size_t q = (size_t)n;
    return selftest_run(c, "selftest_seed",
                        {{v, nullptr, q * 4}, {L, nullptr, q * 4}, {flags, nullptr, q * 4}, {x, nullptr, q * 24},
                         {nullptr, out, q * 20}},
                        [&](const std::vector<void *> &p) {
                            return launch_selftest_seed(n, (const float *)p[0], (const float *)p[1], (const uint32_t *)p[2],
                                                        (const uint32_t *)p[3], (uint32_t *)p[4], c->stream);
                        });
}

int ksched_selftest_touch_screen(ksched_ctx *c, int64_t n, const int64_t *req, const int64_t *alloc, const float *thr,
                                 const uint32_t *active, float *out_f32, uint32_t *out_u32, double *out_key) {
    if (!c || n < 0 || (n > 0 && (!req || !alloc || !thr || !active || !out_f32 || !out_u32 || !out_key)))
        return KSCHED_E_INVALID;
    if (n == 0) return KSCHED_OK;
    const size_t q = (size_t)n;
    return selftest_run(c, "selftest_touch_screen",
                        {{req, nullptr, q * 24}, {alloc, nullptr, q * 24}, {thr, nullptr, q * 4}, {active, nullptr, q * 4},
                         {nullptr, out_f32, q * 16}, {nullptr, out_u32, q * 8}, {nullptr, out_key, q * 8}},
                        [&](const std::vector<void *> &p) {
                            return launch_selftest_touch_screen(n, (const int64_t *)p[0], (const int64_t *)p[1],
                                                                (const float *)p[2], (const uint32_t *)p[3], (float *)p[4],
                                                                (uint32_t *)p[5], (double *)p[6], c->stream);
                        });
}

int ksched_selftest_wave(ksched_ctx *c, int64_t ncases, const uint64_t *sort_code, const int32_t *sort_idx,
                         const double *key, const int32_t *idx, const int32_t *aux, const int32_t *cut,
                         const int32_t *nv, uint64_t *out_u64, int32_t *out_i32) {
    if (!c || ncases < 0 || ncases > (1 << 20) ||
        (ncases > 0 && (!sort_code || !sort_idx || !key || !idx || !aux || !cut || !nv || !out_u64 || !out_i32)))
        return KSCHED_E_INVALID;
    if (ncases == 0) return KSCHED_OK;
    const size_t l = (size_t)ncases * 64;
    return selftest_run(c, "selftest_wave",
                        {{sort_code, nullptr, l * 6 * 8}, {sort_idx, nullptr, l * 6 * 4}, {key, nullptr, l * 8},
                         {idx, nullptr, l * 4}, {aux, nullptr, l * 4}, {cut, nullptr, (size_t)ncases * 4},
                         {nv, nullptr, (size_t)ncases * 4}, {nullptr, out_u64, l * 12 * 8}, {nullptr, out_i32, l * 13 * 4}},
                        [&](const std::vector<void *> &p) {
                            WaveTestArgs a{};
                            a.ncases = ncases;
                            a.scode = (const uint64_t *)p[0]; a.sidx = (const int32_t *)p[1];
                            a.key = (const double *)p[2]; a.kidx = (const int32_t *)p[3]; a.aux = (const int32_t *)p[4];
                            a.cut = (const int32_t *)p[5]; a.nv = (const int32_t *)p[6];
                            uint64_t *u = (uint64_t *)p[7];
                            int32_t *v = (int32_t *)p[8];
                            a.ocode = u; a.red_max = u + 6 * l; a.red_sum = (int64_t *)(u + 7 * l);
                            a.ab_key = u + 8 * l; a.kcode = u + 10 * l; a.red_or = u + 11 * l;
                            a.oidx = v; a.rank = v + 6 * l; a.red_min = v + 7 * l; a.ab_idx = v + 8 * l;
                            a.ab_aux = v + 10 * l; a.thr = v + 12 * l;
                            return launch_selftest_wave(a, c->stream);
                        });
}

int ksched_selftest_list(ksched_ctx *c, int64_t n, int32_t steps, const double *key, const int32_t *idx,
                         double *out_key, int32_t *out_idx) {
    if (!c || n < 0 || steps < 0 || steps > 4096 || (n > 0 && (!out_key || !out_idx)) ||
        (n > 0 && steps > 0 && (!key || !idx)))
        return KSCHED_E_INVALID;
    if (n == 0) return KSCHED_OK;
    const size_t q = (size_t)n;
    return selftest_run(c, "selftest_list",
                        {{key, nullptr, q * (size_t)steps * 8}, {idx, nullptr, q * (size_t)steps * 4},
                         {nullptr, out_key, q * 30 * 8}, {nullptr, out_idx, q * 30 * 4}},
                        [&](const std::vector<void *> &p) {
                            return launch_selftest_list(n, steps, (const double *)p[0], (const int32_t *)p[1],
                                                        (double *)p[2], (int32_t *)p[3], c->stream);
                        });
}

int ksched_selftest_slots(ksched_ctx *c, int64_t n, int32_t steps, const uint32_t *x, uint32_t *out) {
    if (!c || n < 0 || steps < 0 || steps > 4096 || (n > 0 && !out) || (n > 0 && steps > 0 && !x)) return KSCHED_E_INVALID;
    if (n == 0) return KSCHED_OK;
    const size_t q = (size_t)n;
    return selftest_run(c, "selftest_slots", {{x, nullptr, q * (size_t)steps * 2 * 4 * 4}, {nullptr, out, q * 60 * 4}},
                        [&](const std::vector<void *> &p) {
                            return launch_selftest_slots(n, steps, (const uint32_t *)p[0], (uint32_t *)p[1], c->stream);
                        });
}

// Ranked dry run (ksched_rank.hip).  Touches nothing a schedule call left behind: its pods, span lists and
// outputs live in d->rws, and FAST53 is decided here for these m pods alone (c->fast53 stays the last run's).
int ksched_rank(ksched_ctx *c, int64_t m, const int64_t *rc, const int64_t *rm, const int64_t *rp, const uint64_t *sel,
                int32_t k, int32_t *out_idx, double *out_score, uint8_t *out_reason, int32_t *out_count,
                int32_t *out_feasible) {
    if (!c) return KSCHED_E_INVALID;
    if (c->n_local < 0) return fail(c, KSCHED_E_STATE, "rank before load_nodes");
    static_assert(KSCHED_RANK_MAX == kRankList, "one list entry per lane");
    if (k < 1 || k > KSCHED_RANK_MAX) return fail(c, KSCHED_E_INVALID, "rank: k must be in 1..KSCHED_RANK_MAX");
    if (m < 0 || (m > 0 && (!rc || !rm || !rp))) return fail(c, KSCHED_E_INVALID, "rank: bad arguments");
    if (c->o.use_labels && m > 0 && !sel) return fail(c, KSCHED_E_INVALID, "rank: use_labels needs selectors");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (m == 0) return KSCHED_OK;
    const int64_t n = c->n_local;
    if (n == 0) {  // an empty shard ranks nothing
        const size_t e = (size_t)m * (size_t)k;
        if (out_idx) std::fill(out_idx, out_idx + e, -1);
        if (out_score) std::fill(out_score, out_score + e, 0.0);
        if (out_reason) std::memset(out_reason, 0, e);
        if (out_count) std::fill(out_count, out_count + m, 0);
        if (out_feasible) std::fill(out_feasible, out_feasible + m, 0);
        return KSCHED_OK;
    }
    uint64_t mxr = 0;
    for (int64_t i = 0; i < m; ++i) mxr = std::max(mxr, std::max(uabs(rc[i]), std::max(uabs(rm[i]), uabs(rp[i]))));
    const bool f53 = sat_add(c->max_abs_alloc, mxr) < (1ull << 52);
    // the workspace of one chunk: pods | span lists | counts | outputs, each 256-byte aligned
    const int64_t mc_max = std::min<int64_t>(m, kRankChunk);
    size_t nl = 0;  // span lists of the largest chunk: at most kRankGridWGs * kRankTile (rank_geometry)
    for (int64_t q : {mc_max, m % kRankChunk}) {  // the full chunk and the tail (fewer pods, more spans)
        if (q <= 0) continue;
        int32_t s; int64_t rows;
        rank_geometry(n, q, &s, &rows);
        nl = std::max(nl, (size_t)q * (size_t)s);
    }
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t o_pods = 0, o_part = al(o_pods + (size_t)mc_max * 32), o_fc = al(o_part + nl * kRankList * sizeof(Cand)),
                 o_idx = al(o_fc + nl * 4), o_sc = al(o_idx + (size_t)mc_max * k * 4), o_rs = al(o_sc + (size_t)mc_max * k * 8),
                 o_cnt = al(o_rs + (size_t)mc_max * k), o_feas = al(o_cnt + (size_t)mc_max * 4),
                 total = al(o_feas + (size_t)mc_max * 4);
    HIPCHK(c, c->d->rws.reserve(total));
    char *w = static_cast<char *>(c->d->rws.p);
    std::vector<char> stage(std::max((size_t)mc_max * 32, total - o_idx));  // host side of the chunk's two copies
    for (int64_t at = 0; at < m; at += kRankChunk) {
        const int64_t mc = std::min<int64_t>(kRankChunk, m - at);
        RankArgs a{};
        a.nodes = c->d->nodes; a.n_local = n; a.node_offset = c->o.node_offset;
        int64_t *dp = reinterpret_cast<int64_t *>(w + o_pods);
        a.rc = dp; a.rm = dp + mc; a.rp = dp + 2 * mc; a.sel = reinterpret_cast<uint64_t *>(dp + 3 * mc);
        a.m = (int32_t)mc; a.k = k;
        rank_geometry(n, mc, &a.spans, &a.span_rows);
        if ((size_t)mc * a.spans > nl) return fail(c, KSCHED_E_NOMEM, "rank: workspace bound");  // (rank_geometry's bound)
        a.part = reinterpret_cast<Cand *>(w + o_part); a.part_fc = reinterpret_cast<int32_t *>(w + o_fc);
        a.out_idx = reinterpret_cast<int32_t *>(w + o_idx); a.out_score = reinterpret_cast<double *>(w + o_sc);
        a.out_reason = reinterpret_cast<uint8_t *>(w + o_rs); a.out_count = reinterpret_cast<int32_t *>(w + o_cnt);
        a.out_feasible = reinterpret_cast<int32_t *>(w + o_feas);
        // one copy in and one copy out per chunk (a one-pod call is mostly copies), in the stream of the kernels
        int64_t *hp = reinterpret_cast<int64_t *>(stage.data());
        std::memcpy(hp, rc + at, (size_t)mc * 8);
        std::memcpy(hp + mc, rm + at, (size_t)mc * 8);
        std::memcpy(hp + 2 * mc, rp + at, (size_t)mc * 8);
        if (sel) std::memcpy(hp + 3 * mc, sel + at, (size_t)mc * 8);
        else std::memset(hp + 3 * mc, 0, (size_t)mc * 8);
        HIPCHK(c, hipMemcpyAsync(dp, hp, (size_t)mc * 32, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_rank(c->o.priority, c->o.domain, c->o.use_labels != 0, f53, a, c->stream));
        HIPCHK(c, hipMemcpyAsync(stage.data(), w + o_idx, total - o_idx, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // the next chunk reuses the workspace and the staging buffer
        const size_t e = (size_t)mc * k, eo = (size_t)at * k;
        const char *ho = stage.data();  // the outputs, at their workspace offsets less o_idx
        if (out_idx) std::memcpy(out_idx + eo, ho, e * 4);
        if (out_score) std::memcpy(out_score + eo, ho + (o_sc - o_idx), e * 8);
        if (out_reason) std::memcpy(out_reason + eo, ho + (o_rs - o_idx), e);
        if (out_count) std::memcpy(out_count + at, ho + (o_cnt - o_idx), (size_t)mc * 4);
        if (out_feasible) std::memcpy(out_feasible + at, ho + (o_feas - o_idx), (size_t)mc * 4);
    }
    return KSCHED_OK;
}

// Host only: the shards' ranked lists -> the global one, in the same order (key descending = score descending, or
// price ascending; global index ascending on ties), by an R-way merge of the list heads.
int ksched_rank_merge(int32_t priority, int32_t nranks, int64_t m, int32_t k, const int32_t *idx_all,
                      const double *score_all, const uint8_t *reason_all, const int32_t *count_all,
                      const int32_t *feasible_all, int32_t *out_idx, double *out_score, uint8_t *out_reason,
                      int32_t *out_count, int32_t *out_feasible) {
    if (priority != KSCHED_PRIORITY_RESOURCE && priority != KSCHED_PRIORITY_BEST_PRICE) return KSCHED_E_INVALID;
    if (nranks < 1 || k < 1 || k > KSCHED_RANK_MAX || m < 0) return KSCHED_E_INVALID;
    if (m > 0 && (!idx_all || !score_all || !count_all)) return KSCHED_E_INVALID;
    const bool price = priority == KSCHED_PRIORITY_BEST_PRICE;
    std::vector<int32_t> head((size_t)nranks);
    for (int64_t i = 0; i < m; ++i) {
        int64_t feas = 0;
        for (int32_t r = 0; r < nranks; ++r) {
            head[(size_t)r] = 0;
            const int32_t cn = count_all[(size_t)r * m + i];
            if (cn < 0 || cn > k) return KSCHED_E_INVALID;
            if (feasible_all) feas += feasible_all[(size_t)r * m + i];
        }
        int32_t q = 0;
        for (; q < k; ++q) {
            int32_t br = -1;
            size_t be = 0;
            for (int32_t r = 0; r < nranks; ++r) {
                if (head[(size_t)r] >= count_all[(size_t)r * m + i]) continue;
                const size_t e = ((size_t)r * m + i) * k + head[(size_t)r];
                if (br >= 0) {
                    const double a = score_all[e], b = score_all[be];
                    const bool bt = price ? a < b : a > b;
                    if (!(bt || (a == b && idx_all[e] < idx_all[be]))) continue;
                }
                br = r; be = e;
            }
            if (br < 0) break;
            ++head[(size_t)br];
            const size_t o = (size_t)i * k + q;
            if (out_idx) out_idx[o] = idx_all[be];
            if (out_score) out_score[o] = score_all[be];
            if (out_reason) out_reason[o] = reason_all ? reason_all[be] : 0;
        }
        if (out_count) out_count[i] = q;
        for (; q < k; ++q) {
            const size_t o = (size_t)i * k + q;
            if (out_idx) out_idx[o] = -1;
            if (out_score) out_score[o] = 0.0;
            if (out_reason) out_reason[o] = 0;
        }
        if (out_feasible) out_feasible[i] = (int32_t)feas;
    }
    return KSCHED_OK;
}

}  // extern "C"

// The six output columns of ksched_preempt and ksched_preempt_constrained (any pointer may be null).
namespace {
struct PreemptOut {
    int32_t *node, *nvictims, *max_prio;
    int64_t *sum_prio;
    int32_t *candidates, *victims;
    // m pods without a candidate
    void no_candidate(int64_t m, int32_t vcap) const {
        if (node) std::fill(node, node + m, KSCHED_NO_FIT);
        if (nvictims) std::fill(nvictims, nvictims + m, 0);
        if (max_prio) std::fill(max_prio, max_prio + m, KSCHED_PREEMPT_NO_VICTIM_PRIO);
        if (sum_prio) std::fill(sum_prio, sum_prio + m, (int64_t)0);
        if (candidates) std::fill(candidates, candidates + m, 0);
        if (victims) std::fill(victims, victims + (size_t)m * vcap, -1);
    }
    // a chunk's mc pods from pod `at` on, out of its staged copy: ho holds the node column, the others at these offsets
    void chunk(int64_t at, int64_t mc, int32_t vcap, const char *ho, size_t nv, size_t mx, size_t sum, size_t cand, size_t vic) const {
        if (node) std::memcpy(node + at, ho, (size_t)mc * 4);
        if (nvictims) std::memcpy(nvictims + at, ho + nv, (size_t)mc * 4);
        if (max_prio) std::memcpy(max_prio + at, ho + mx, (size_t)mc * 4);
        if (sum_prio) std::memcpy(sum_prio + at, ho + sum, (size_t)mc * 8);
        if (candidates) std::memcpy(candidates + at, ho + cand, (size_t)mc * 4);
        if (victims) std::memcpy(victims + (size_t)at * vcap, ho + vic, (size_t)mc * vcap * 4);
    }
};
}  // namespace

// The bound-pod table of ksched_preempt and ksched_preempt_constrained: built on the host (build_bound_table; x's extra
// columns beside it, pc_pack_columns), uploaded in the stream of the kernels that read it.  Touches no node row; the
// context holds no table until the last copy has landed.  The arguments have passed the caller's checks.
static int load_bound_table(ksched_ctx *c, const std::string &nm, const PcBound &x) {
    BoundTableHost h;
    std::vector<int64_t> hext;
    std::vector<uint64_t> hmask;
    uint64_t mask_or = 0;
    const char *why = "";
    try {
        if (!build_bound_table(c->n_local, x.nb, x.node_idx, x.cpu, x.mem, x.prio, &h, &why))
            return fail(c, KSCHED_E_INVALID, nm + ": " + why);
        if (x.n_ext > 0 || x.bound_spread) pc_pack_columns(h.tidx, x, &hext, &hmask, &mask_or);
    } catch (const std::bad_alloc &) {
        return fail(c, KSCHED_E_NOMEM, nm + ": host allocation of the table failed");
    }
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->bound_valid = false;
    ksched_bufs &d = *c->d;
    const size_t e = h.cpu.size(), nblk = h.off.size(), n = h.seg.size();
    hipError_t r = d.bcpu.reserve(e * 8);
    if (r == hipSuccess) r = d.bmem.reserve(e * 8);
    if (r == hipSuccess) r = d.bprio.reserve(e * 4);
    if (r == hipSuccess) r = d.btidx.reserve(e * 4);
    if (r == hipSuccess) r = d.boff.reserve(nblk * 8);
    if (r == hipSuccess) r = d.bdepth.reserve(nblk * 4);
    if (r == hipSuccess) r = d.bseg.reserve(n * 4);
    if (r == hipSuccess && x.n_ext > 0) r = d.bext.reserve(hext.size() * 8);
    if (r == hipSuccess && x.bound_spread) r = d.bmask.reserve(e * 8);
    if (r != hipSuccess) {
        (void)hipGetLastError();
        if (r == hipErrorOutOfMemory) return fail(c, KSCHED_E_NOMEM, nm + ": device allocation of the table failed");
        return fail(c, KSCHED_E_DEVICE, nm + ": " + hipGetErrorString(r));
    }
    auto up = [&](void *dst, const void *src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    };
    HIPCHK(c, up(d.bcpu, h.cpu.data(), e * 8)); HIPCHK(c, up(d.bmem, h.mem.data(), e * 8));
    HIPCHK(c, up(d.bprio, h.prio.data(), e * 4)); HIPCHK(c, up(d.btidx, h.tidx.data(), e * 4));
    HIPCHK(c, up(d.boff, h.off.data(), nblk * 8)); HIPCHK(c, up(d.bdepth, h.depth.data(), nblk * 4));
    HIPCHK(c, up(d.bseg, h.seg.data(), n * 4));
    if (x.n_ext > 0) HIPCHK(c, up(d.bext, hext.data(), hext.size() * 8));
    if (x.bound_spread) HIPCHK(c, up(d.bmask, hmask.data(), e * 8));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the host vectors go away with this call
    c->bound_R = x.n_ext; c->bound_mask_or = mask_or; c->bound_entries = (int64_t)e; c->bound_mask_dev = x.bound_spread != nullptr;
    c->bound_valid = true;
    return KSCHED_OK;
}

extern "C" {

int ksched_load_bound(ksched_ctx *c, int64_t nb, const int32_t *node_idx, const int64_t *cpu, const int64_t *mem,
                      const int32_t *prio) {
    if (!c) return KSCHED_E_INVALID;
    if (c->n_local < 0) return fail(c, KSCHED_E_STATE, "load_bound before load_nodes");
    static_assert(KSCHED_BOUND_MAX_PER_NODE == kBoundMaxPerNode, "segment bound");
    if (nb < 0 || nb >= 0x7fffffff || (nb > 0 && (!node_idx || !cpu || !mem || !prio)))
        return fail(c, KSCHED_E_INVALID, "load_bound: bad arguments");
    return load_bound_table(c, "load_bound", PcBound{nb, node_idx, cpu, mem, prio, 0, nullptr, nullptr});
}

// ksched_load_bound with the table's two extra columns (ksched_preemptc.h has the checks and the packing).
int ksched_load_bound_constrained(ksched_ctx *c, int64_t nb, const int32_t *node_idx, const int64_t *cpu, const int64_t *mem,
                                  const int32_t *prio, int32_t n_ext, const int64_t *bound_ext, const uint64_t *bound_spread) {
    if (!c) return KSCHED_E_INVALID;
    if (c->n_local < 0) return fail(c, KSCHED_E_STATE, "load_bound_constrained before load_nodes");
    const PcBound x{nb, node_idx, cpu, mem, prio, n_ext, bound_ext, bound_spread};
    try {
        if (const char *why = pc_check_bound(x, c->n_local)) return fail(c, KSCHED_E_INVALID, std::string("load_bound_constrained: ") + why);
    } catch (const std::bad_alloc &) {
        return fail(c, KSCHED_E_NOMEM, "load_bound_constrained: host allocation failed");
    }
    return load_bound_table(c, "load_bound_constrained", x);
}

// Preemption dry run (ksched_preempt.hip).  As ksched_rank: its pods, span parts and outputs live in a workspace of its
// own (d->vws), one chunk of kPreemptChunk pods at a time; nothing a schedule call left behind is touched.
int ksched_preempt(ksched_ctx *c, int64_t m, const int64_t *rc, const int64_t *rm, const int64_t *rp, const uint64_t *sel,
                   const int32_t *prio, int32_t vcap, int32_t *out_node, int32_t *out_nvictims, int32_t *out_max_prio,
                   int64_t *out_sum_prio, int32_t *out_candidates, int32_t *out_victims) {
    if (!c) return KSCHED_E_INVALID;
    if (c->n_local < 0) return fail(c, KSCHED_E_STATE, "preempt before load_nodes");
    if (vcap < 1 || vcap > KSCHED_BOUND_MAX_PER_NODE)
        return fail(c, KSCHED_E_INVALID, "preempt: vcap must be in 1..KSCHED_BOUND_MAX_PER_NODE");
    if (m < 0 || (m > 0 && (!rc || !rm || !rp || !prio))) return fail(c, KSCHED_E_INVALID, "preempt: bad arguments");
    if (c->o.use_labels && m > 0 && !sel) return fail(c, KSCHED_E_INVALID, "preempt: use_labels needs selectors");
    if (!c->bound_valid) return fail(c, KSCHED_E_STATE, "preempt: no bound-pod table (ksched_load_bound after every ksched_load_nodes)");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (m == 0) return KSCHED_OK;
    const int64_t n = c->n_local;
    if (n == 0) {  // an empty shard has no candidate
        const PreemptOut out{out_node, out_nvictims, out_max_prio, out_sum_prio, out_candidates, out_victims};
        out.no_candidate(m, vcap);
        return KSCHED_OK;
    }
    // the workspace of one chunk: pods | span parts | counts | outputs, each 256-byte aligned
    const int64_t mc_max = std::min<int64_t>(m, kPreemptChunk);
    size_t np = 0;  // span parts of the largest chunk: at most kPreemptGridWGs * kPreemptTile (preempt_geometry)
    for (int64_t q : {mc_max, m % kPreemptChunk}) {  // the full chunk and the tail (fewer pods, more spans)
        if (q <= 0) continue;
        int32_t s; int64_t rows;
        preempt_geometry(n, q, &s, &rows);
        np = std::max(np, (size_t)q * (size_t)s);
    }
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t q = (size_t)mc_max;
    const size_t o_pods = 0, o_part = al(o_pods + q * 36), o_nc = al(o_part + np * sizeof(PreemptPart)),
                 o_node = al(o_nc + np * 4), o_nv = al(o_node + q * 4), o_mx = al(o_nv + q * 4), o_sum = al(o_mx + q * 4),
                 o_cand = al(o_sum + q * 8), o_vic = al(o_cand + q * 4), total = al(o_vic + q * (size_t)vcap * 4);
    HIPCHK(c, c->d->vws.reserve(total));
    char *w = static_cast<char *>(c->d->vws.p);
    // the victims leave only when asked for: up to 4 MiB of the chunk's copy out
    const size_t out_bytes = (out_victims ? total : o_vic) - o_node;
    std::vector<char> stage(std::max(q * 36, out_bytes));  // host side of the chunk's two copies
    const ksched_bufs &d = *c->d;
    for (int64_t at = 0; at < m; at += kPreemptChunk) {
        const int64_t mc = std::min<int64_t>(kPreemptChunk, m - at);
        PreemptArgs a{};
        a.nodes = d.nodes; a.n_local = n; a.node_offset = c->o.node_offset;
        a.tb.cpu = d.bcpu; a.tb.mem = d.bmem; a.tb.prio = d.bprio; a.tb.tidx = d.btidx;
        a.tb.off = d.boff; a.tb.depth = d.bdepth; a.tb.seg = d.bseg;
        int64_t *dp = reinterpret_cast<int64_t *>(w + o_pods);
        a.rc = dp; a.rm = dp + mc; a.rp = dp + 2 * mc; a.sel = reinterpret_cast<uint64_t *>(dp + 3 * mc);
        a.prio = reinterpret_cast<int32_t *>(dp + 4 * mc);
        a.m = (int32_t)mc; a.vcap = vcap;
        preempt_geometry(n, mc, &a.spans, &a.span_rows);
        if ((size_t)mc * a.spans > np) return fail(c, KSCHED_E_NOMEM, "preempt: workspace bound");  // (preempt_geometry's bound)
        a.part = reinterpret_cast<PreemptPart *>(w + o_part); a.part_nc = reinterpret_cast<int32_t *>(w + o_nc);
        a.out_node = reinterpret_cast<int32_t *>(w + o_node); a.out_nvictims = reinterpret_cast<int32_t *>(w + o_nv);
        a.out_max_prio = reinterpret_cast<int32_t *>(w + o_mx); a.out_sum_prio = reinterpret_cast<int64_t *>(w + o_sum);
        a.out_candidates = reinterpret_cast<int32_t *>(w + o_cand); a.out_victims = reinterpret_cast<int32_t *>(w + o_vic);
        // one copy in and one copy out per chunk, in the stream of the kernels
        int64_t *hp = reinterpret_cast<int64_t *>(stage.data());
        std::memcpy(hp, rc + at, (size_t)mc * 8);
        std::memcpy(hp + mc, rm + at, (size_t)mc * 8);
        std::memcpy(hp + 2 * mc, rp + at, (size_t)mc * 8);
        if (sel) std::memcpy(hp + 3 * mc, sel + at, (size_t)mc * 8);
        else std::memset(hp + 3 * mc, 0, (size_t)mc * 8);
        std::memcpy(hp + 4 * mc, prio + at, (size_t)mc * 4);
        HIPCHK(c, hipMemcpyAsync(dp, hp, (size_t)mc * 36, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_preempt(c->o.use_labels != 0, a, c->stream));
        // (a short chunk's victims are [mc][vcap] from o_vic: the copy covers them)
        const size_t cp = out_victims ? (o_vic - o_node) + (size_t)mc * vcap * 4 : out_bytes;
        HIPCHK(c, hipMemcpyAsync(stage.data(), w + o_node, cp, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // the next chunk reuses the workspace and the staging buffer
        const PreemptOut out{out_node, out_nvictims, out_max_prio, out_sum_prio, out_candidates, out_victims};
        out.chunk(at, mc, vcap, stage.data(), o_nv - o_node, o_mx - o_node, o_sum - o_node, o_cand - o_node, o_vic - o_node);
    }
    return KSCHED_OK;
}

// Preemption dry run under the extended columns and the spread table (ksched_preemptc.hip).  ksched_preempt's shape:
// the groups' minima, one chunk's pods, span parts and outputs live in a workspace of its own (d->cws); every check
// (ksched_preemptc.h) runs before anything is allocated or staged; nothing a schedule call left behind is touched.
int ksched_preempt_constrained(ksched_ctx *c, int64_t m, const int64_t *rc, const int64_t *rm, const int64_t *rp,
                               const uint64_t *sel, const int32_t *prio, const int32_t *spread_group,
                               const uint8_t *spread_enforce, const int64_t *req_ext, int32_t vcap, int32_t *out_node,
                               int32_t *out_nvictims, int32_t *out_max_prio, int64_t *out_sum_prio, int32_t *out_candidates,
                               int32_t *out_victims) {
    if (!c) return KSCHED_E_INVALID;
    PcPacked k;
    try {
        const PcCall call{m, rc, rm, rp, sel, prio, spread_group, spread_enforce, req_ext, vcap};
        const PcState st{c->n_local >= 0, c->o.use_labels != 0, c->o.nranks, c->bound_valid, c->bound_R, c->bound_mask_or,
                         c->spread_S, c->ext_R};
        const char *why = nullptr;
        if (const int code = pc_check_pack(call, st, &k, &why)) return fail(c, code, std::string("preempt_constrained: ") + why);
    } catch (const std::bad_alloc &) {
        return fail(c, KSCHED_E_NOMEM, "preempt_constrained: host staging buffer");
    }
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (m == 0) return KSCHED_OK;
    const int64_t n = c->n_local;
    const PreemptOut out{out_node, out_nvictims, out_max_prio, out_sum_prio, out_candidates, out_victims};
    if (n == 0) {  // no node, no candidate
        out.no_candidate(m, vcap);
        return KSCHED_OK;
    }
    ksched_bufs &d = *c->d;
    if (k.spread && !c->bound_mask_dev) {  // a table without masks: the column of zeros it stands for
        HIPCHK(c, d.bmask.reserve((size_t)c->bound_entries * 8));
        if (c->bound_entries > 0) HIPCHK(c, hipMemsetAsync(d.bmask, 0, (size_t)c->bound_entries * 8, c->stream));
        c->bound_mask_dev = true;
    }
    // the workspace: minima | one chunk's pods | span parts | counts | outputs, each 256-byte aligned
    const int64_t mc_max = std::min<int64_t>(m, kPreemptChunk);
    size_t np = 0;  // span parts of the largest chunk: at most kPreemptGridWGs * kPreemptCTile (preemptc_geometry)
    for (int64_t q : {mc_max, m % kPreemptChunk}) {  // the full chunk and the tail (fewer pods, more spans)
        if (q <= 0) continue;
        int32_t s; int64_t rows;
        preemptc_geometry(n, q, &s, &rows);
        np = std::max(np, (size_t)q * (size_t)s);
    }
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t q = (size_t)mc_max;
    constexpr size_t kPod = 36 + KSCHED_EXT_MAX * 8 + 4;  // rc | rm | rp | sel | er[4] | prio | sg per pod
    const size_t o_min = 0, o_pods = al(o_min + (size_t)KSCHED_SPREAD_MAX_GROUPS * kPreemptCMinWords * 4),
                 o_part = al(o_pods + q * kPod), o_nc = al(o_part + np * sizeof(PreemptPart)),
                 o_node = al(o_nc + np * 4), o_nv = al(o_node + q * 4), o_mx = al(o_nv + q * 4), o_sum = al(o_mx + q * 4),
                 o_cand = al(o_sum + q * 8), o_vic = al(o_cand + q * 4), total = al(o_vic + q * (size_t)vcap * 4);
    HIPCHK(c, d.cws.reserve(total));
    char *w = static_cast<char *>(d.cws.p);
    PreemptCArgs A{};
    A.bext = d.bext; A.entries = c->bound_entries; A.bmask = d.bmask;
    if (k.ext) { A.ext = d.etab; A.n_ext = c->ext_R; }
    if (k.spread) { A.sp_dom = d.sdom; A.sp_cnt = d.scnt; A.sp_skew = d.sskew; A.sp_D = c->spread_D; A.sp_S = c->spread_S; }
    A.sp_min = reinterpret_cast<int32_t *>(w + o_min);
    HIPCHK(c, launch_preemptc_min(A, c->stream));
    // the victims leave only when asked for: up to 4 MiB of the chunk's copy out
    const size_t out_bytes = (out_victims ? total : o_vic) - o_node;
    std::vector<char> stage(std::max(q * kPod, out_bytes));  // host side of the chunk's two copies
    for (int64_t at = 0; at < m; at += kPreemptChunk) {
        const int64_t mc = std::min<int64_t>(kPreemptChunk, m - at);
        PreemptArgs &a = A.a;
        a = PreemptArgs{};
        a.nodes = d.nodes; a.n_local = n; a.node_offset = c->o.node_offset;
        a.tb.cpu = d.bcpu; a.tb.mem = d.bmem; a.tb.prio = d.bprio; a.tb.tidx = d.btidx;
        a.tb.off = d.boff; a.tb.depth = d.bdepth; a.tb.seg = d.bseg;
        int64_t *dp = reinterpret_cast<int64_t *>(w + o_pods);
        a.rc = dp; a.rm = dp + mc; a.rp = dp + 2 * mc; a.sel = reinterpret_cast<uint64_t *>(dp + 3 * mc);
        A.er = dp + 4 * mc;
        a.prio = reinterpret_cast<int32_t *>(dp + (4 + KSCHED_EXT_MAX) * mc);
        A.sg = a.prio + mc;
        a.m = (int32_t)mc; a.vcap = vcap;
        preemptc_geometry(n, mc, &a.spans, &a.span_rows);
        if ((size_t)mc * a.spans > np) return fail(c, KSCHED_E_NOMEM, "preempt_constrained: workspace bound");  // (preemptc_geometry's bound)
        a.part = reinterpret_cast<PreemptPart *>(w + o_part); a.part_nc = reinterpret_cast<int32_t *>(w + o_nc);
        a.out_node = reinterpret_cast<int32_t *>(w + o_node); a.out_nvictims = reinterpret_cast<int32_t *>(w + o_nv);
        a.out_max_prio = reinterpret_cast<int32_t *>(w + o_mx); a.out_sum_prio = reinterpret_cast<int64_t *>(w + o_sum);
        a.out_candidates = reinterpret_cast<int32_t *>(w + o_cand); a.out_victims = reinterpret_cast<int32_t *>(w + o_vic);
        // one copy in and one copy out per chunk, in the stream of the kernels
        int64_t *hp = reinterpret_cast<int64_t *>(stage.data());
        std::memcpy(hp, rc + at, (size_t)mc * 8);
        std::memcpy(hp + mc, rm + at, (size_t)mc * 8);
        std::memcpy(hp + 2 * mc, rp + at, (size_t)mc * 8);
        if (sel) std::memcpy(hp + 3 * mc, sel + at, (size_t)mc * 8);
        else std::memset(hp + 3 * mc, 0, (size_t)mc * 8);
        std::memcpy(hp + 4 * mc, k.er.data() + (size_t)at * KSCHED_EXT_MAX, (size_t)mc * KSCHED_EXT_MAX * 8);
        int32_t *hq = reinterpret_cast<int32_t *>(hp + (4 + KSCHED_EXT_MAX) * mc);
        std::memcpy(hq, prio + at, (size_t)mc * 4);
        std::memcpy(hq + mc, k.sg.data() + at, (size_t)mc * 4);
        HIPCHK(c, hipMemcpyAsync(dp, hp, (size_t)mc * kPod, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_preemptc(c->o.use_labels != 0, A, c->stream));
        // (a short chunk's victims are [mc][vcap] from o_vic: the copy covers them)
        const size_t cp = out_victims ? (o_vic - o_node) + (size_t)mc * vcap * 4 : out_bytes;
        HIPCHK(c, hipMemcpyAsync(stage.data(), w + o_node, cp, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // the next chunk reuses the workspace and the staging buffer
        out.chunk(at, mc, vcap, stage.data(), o_nv - o_node, o_mx - o_node, o_sum - o_node, o_cand - o_node, o_vic - o_node);
    }
    return KSCHED_OK;
}

int ksched_download_results(ksched_ctx *c, int64_t p, int32_t *oi, double *os, int32_t *of) {
    if (!c) return KSCHED_E_INVALID;
    if (p != c->p) return fail(c, KSCHED_E_INVALID, "download_results: size mismatch");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (p == 0) return KSCHED_OK;
    if (oi) HIPCHK(c, hipMemcpy(oi, c->d->oidx, (size_t)p * 4, hipMemcpyDeviceToHost));
    if (os) HIPCHK(c, hipMemcpy(os, c->d->osc, (size_t)p * 8, hipMemcpyDeviceToHost));
    if (of) HIPCHK(c, hipMemcpy(of, c->d->ofeas, (size_t)p * 4, hipMemcpyDeviceToHost));
    if (oi && c->st.placed == 0) {
        int64_t placed = 0;
        for (int64_t i = 0; i < p; ++i) placed += oi[i] >= 0;
        c->st.placed = placed;
    }
    return KSCHED_OK;
}

}  // extern "C"

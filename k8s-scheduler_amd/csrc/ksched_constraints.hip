// ksched_constraints.hip -- libksched: the constraints of exact mode above the kernel.  The constrained schedule calls
// (ksched_schedule_*) go one way: each names its kind of k_exact (exact_kind, ksched_exact.h), and schedule_kind checks
// and packs on the host for that kind (ksched_full.h), stages what was packed and runs; the table calls load and read
// the context's spread, extended-resource and affinity tables; the dry runs (ksched_rank_full, ksched_explain_full) read
// the rows and those tables through the kernels of ksched_dryrun.hip and write nothing a context holds.
#include <algorithm>
#include <cstring>

#include <new>
#include <utility>

#include "ksched_affinity.h"
#include "ksched_ctx.h"
#include "ksched_dryrun.h"
#include "ksched_ext.h"
#include "ksched_full.h"
#include "ksched_gang.h"
#include "ksched_spread.h"
#include "ksched_why.h"

using namespace ksched;

namespace {

// The pods' requests and the results' arrays of a schedule call, as include/ksched.h names them.
struct PodIO {
    const int64_t *rc, *rm, *rp;
    const uint64_t *sel;
    int32_t *oi;
    double *os;
    int32_t *of;
};

// One array a call stages for the kernel where its kind carries the array's constraint (on): the context's buffer, the
// packed host array (null: an output of the kernel, reserved only) and its bytes.
template <class T>
struct Staged {
    bool on;
    DevBuf<T> &buf;
    const T *host;
    size_t bytes;
};

// What the schedule calls share once their checks have passed and their arrays are packed: the pods go up, the
// staged arrays are reserved and copied in the stream of the kernel that reads them -- finished before the host arrays
// go (ksched_upload_pods) -- then the run over them, the sync on both outcomes, and the results.
template <class... S>
int schedule_staged(ksched_ctx *c, ExactRun run, const char *name, int64_t p, const PodIO &io, const S &...staged) {
    int r = ksched_upload_pods(c, p, io.rc, io.rm, io.rp, io.sel);
    if (r != KSCHED_OK) return r;
    hipError_t e = hipSuccess;
    auto reserve = [&](const auto &st) { if (st.on && e == hipSuccess) e = st.buf.reserve(st.bytes); };
    auto copy = [&](const auto &st) {
        if (st.on && e == hipSuccess && st.host && st.bytes > 0)
            e = hipMemcpyAsync(st.buf, st.host, st.bytes, hipMemcpyHostToDevice, c->stream);
    };
    (reserve(staged), ...);  // every array reserved before the first is copied; a step runs only if the last succeeded
    (copy(staged), ...);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, KSCHED_E_DEVICE, std::string(name) + ": staging: " + hipGetErrorString(e));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((r = run_impl(c, run)) != KSCHED_OK) { ksched_sync(c); return r; }
    if ((r = ksched_sync(c)) != KSCHED_OK) return r;
    return ksched_download_results(c, p, io.oi, io.os, io.of);
}

// After a run with gangs: the members bound per gang come down, stats.placed is their sum (a rolled-back member is not
// placed), and the caller gets them where it asked (out may be null).
int gang_results(ksched_ctx *c, size_t ng, int32_t *out) {
    std::vector<int32_t> gp(ng);
    if (ng > 0) HIPCHK(c, hipMemcpy(gp.data(), c->d->gplaced, ng * 4, hipMemcpyDeviceToHost));
    c->st.placed = 0;
    for (int32_t v : gp) c->st.placed += v;
    if (out && ng > 0) std::memcpy(out, gp.data(), ng * 4);
    return KSCHED_OK;
}

static_assert(KSCHED_GANG_MAX == kGangMax && KSCHED_GANG_REJECTED == kGangRejected, "gang constants");
static_assert(KSCHED_NUM_REASONS_FULL == kNumWhyReasons, "why constants");

// The first half of every constrained schedule call, nothing of it on the device: the checks every call shares, then
// the kind's check-and-pack (ksched_full.h).  A refusal leaves the context as it was.
int constrained_begin(ksched_ctx *c, ExactRun run, const char *name, const FullArgs &args, FullPacked *k) {
    if (!c) return KSCHED_E_INVALID;
    const std::string nm(name);
    if (c->n_local < 0) return fail(c, KSCHED_E_STATE, nm + " before load_nodes");
    if (c->o.nranks > 1) return fail(c, KSCHED_E_INVALID, nm + " is single-GPU (the exact kernel)");
    try {
        const char *why = nullptr;
        if (const int code = full_check_pack(exact_kind(run), args, c->spread_S, c->ext_R, c->aff_valid, k, &why))
            return fail(c, code, nm + ": " + why);
    } catch (const std::bad_alloc &) {
        return fail(c, KSCHED_E_NOMEM, nm + ": host staging buffer");
    }
    return KSCHED_OK;
}

// The second half: the run's "on" flags, the arrays of the constraints the kind carries go up, the run over them, the
// results, the final any words where affinity was on and the gangs' counts where the kind has gangs (to the caller only
// where it gave gangs).
int constrained_run(ksched_ctx *c, ExactRun run, const char *name, const FullArgs &args, const FullPacked &k,
                    const PodIO &io, int32_t *out_gang_placed) {
    const ExactKind kind = exact_kind(run);
    const size_t p = (size_t)args.p;
    c->run_spread = k.spread;
    c->run_ext = k.ext;
    c->run_aff = k.aff;
    const int r = schedule_staged(c, run, name, args.p, io,
                                  Staged<int32_t>{kind.gang, c->d->gend, k.gend.data(), p * 4},
                                  Staged<int32_t>{kind.gang, c->d->gplaced, nullptr, k.n_gangs * 4},
                                  Staged<int32_t>{kind.spread, c->d->sword, k.swords.data(), p * 4},
                                  Staged<int64_t>{kind.ext, c->d->ereq, k.reqs.data(), k.reqs.size() * 8},
                                  Staged<int32_t>{kind.ext, c->d->eword, k.ewords.data(), p * 4},
                                  Staged<int32_t>{kind.aff, c->d->aword, k.awords.data(), p * 4},
                                  Staged<uint64_t>{kind.aff, c->d->apod, k.apods.data(), k.apods.size() * 8});
    if (r != KSCHED_OK) return r;
    // the run's final any words, for the next call's arguments (no pods: no launch, the any words stand)
    if (k.aff && args.p > 0) HIPCHK(c, hipMemcpy(c->aff_any, c->d->aany, sizeof(c->aff_any), hipMemcpyDeviceToHost));
    return kind.gang ? gang_results(c, k.n_gangs, args.gang_off ? out_gang_placed : nullptr) : KSCHED_OK;
}

// A constrained schedule call of one kind, whole.  What the kinds do differently is exact_kind's table.
int schedule_kind(ksched_ctx *c, ExactRun run, const char *name, const FullArgs &args, const PodIO &io,
                  int32_t *out_gang_placed) {
    FullPacked k;
    const int r = constrained_begin(c, run, name, args, &k);
    return r != KSCHED_OK ? r : constrained_run(c, run, name, args, k, io, out_gang_placed);
}

// The tables a dry run is given: those its call switched on, as the context holds them (read only), and the workspace
// word per group that k_dry_min fills.
DryTables dry_tables(const ksched_ctx *c, const DryPacked &k, int32_t *sp_min) {
    const ksched_bufs &d = *c->d;
    DryTables t{};
    if (k.spread) { t.sp_dom = d.sdom; t.sp_cnt = d.scnt; t.sp_skew = d.sskew; t.sp_D = c->spread_D; t.sp_S = c->spread_S; t.sp_min = sp_min; }
    if (k.ext) { t.ext = d.etab; t.n_ext = c->ext_R; }
    if (k.aff) { t.af_dom = d.adom; t.af_mem = d.amem; t.af_anti_h = d.aanti_h; t.af_zone = d.azone; t.af_D = c->aff_D; }
    return t;
}

// What both dry runs check before anything else, and the packing of their pods (ksched_dryrun.h).
int dry_begin(ksched_ctx *c, const char *name, const DryCall &call, DryPacked *k) {
    const std::string nm(name);
    if (c->n_local < 0) return fail(c, KSCHED_E_STATE, nm + " before load_nodes");
    if (c->o.nranks > 1) return fail(c, KSCHED_E_INVALID, nm + " is single-GPU (the tables are: there is no shard merge)");
    const DryState st{c->o.use_labels != 0, c->spread_S, c->ext_R, c->aff_valid, c->aff_any[0], c->aff_any[1]};
    try {
        const char *why = nullptr;
        if (const int code = dry_check_pack(call, st, k, &why)) return fail(c, code, nm + ": " + why);
    } catch (const std::bad_alloc &) {
        return fail(c, KSCHED_E_NOMEM, nm + ": host staging buffer");
    }
    return KSCHED_OK;
}

uint64_t uabs64(int64_t v) { return v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v; }

}  // namespace

extern "C" {

// The spread table of ksched_schedule_spread: checked on the host (ksched_spread.h) before anything is allocated or
// staged, then uploaded in the stream of the kernel that reads it.  Touches no node row; the context holds the new
// table only once the last copy has landed, and the earlier one until the checks have passed.
int ksched_load_spread(ksched_ctx *c, int32_t n_domains, const int32_t *node_domain, int32_t n_groups,
                       const int32_t *max_skew, const int32_t *counts) {
    if (!c) return KSCHED_E_INVALID;
    static_assert(KSCHED_SPREAD_MAX_DOMAINS == kSpreadMaxDomains && KSCHED_SPREAD_MAX_GROUPS == kSpreadMaxGroups &&
                  KSCHED_SPREAD_MAX_CELLS == kSpreadMaxCells, "spread constants");
    if (c->n_local < 0) return fail(c, KSCHED_E_STATE, "load_spread before load_nodes");
    if (c->o.nranks > 1) return fail(c, KSCHED_E_INVALID, "load_spread: spread scheduling is single-GPU (the exact kernel)");
    try {
        if (const char *why = spread_check_table(c->n_local, n_domains, node_domain, n_groups, max_skew, counts))
            return fail(c, KSCHED_E_INVALID, std::string("load_spread: ") + why);
    } catch (const std::bad_alloc &) {
        return fail(c, KSCHED_E_NOMEM, "load_spread: host allocation failed");
    }
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->spread_D = c->spread_S = 0;
    ksched_bufs &d = *c->d;
    const size_t n = (size_t)c->n_local, cells = (size_t)n_domains * (size_t)n_groups;
    HIPCHK(c, d.sdom.reserve(n * 4)); HIPCHK(c, d.scnt.reserve(cells * 4)); HIPCHK(c, d.sskew.reserve((size_t)n_groups * 4));
    if (n > 0) HIPCHK(c, hipMemcpyAsync(d.sdom, node_domain, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d.sskew, max_skew, (size_t)n_groups * 4, hipMemcpyHostToDevice, c->stream));
    if (counts) HIPCHK(c, hipMemcpyAsync(d.scnt, counts, cells * 4, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemsetAsync(d.scnt, 0, cells * 4, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's arrays are free again
    c->spread_D = n_domains; c->spread_S = n_groups;
    return KSCHED_OK;
}

int ksched_read_spread(ksched_ctx *c, int32_t *out_counts) {
    if (!c) return KSCHED_E_INVALID;
    if (c->spread_S == 0) return fail(c, KSCHED_E_STATE, "read_spread: no spread table (ksched_load_spread after every ksched_load_nodes)");
    if (!out_counts) return fail(c, KSCHED_E_INVALID, "read_spread: out_counts is NULL");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out_counts, c->d->scnt, (size_t)c->spread_D * (size_t)c->spread_S * 4, hipMemcpyDeviceToHost));
    return KSCHED_OK;
}

// The extended-resource table of ksched_schedule_ext: checked on the host (ksched_ext.h) before anything is allocated,
// then uploaded in the stream of the kernel that reads it.  Touches no node row; the context holds the new table only
// once the copy has landed, and the earlier one until the checks have passed.
int ksched_load_ext(ksched_ctx *c, int32_t n_ext, const int64_t *node_ext) {
    if (!c) return KSCHED_E_INVALID;
    static_assert(KSCHED_EXT_MAX == kExtMax, "ext constants");
    if (c->n_local < 0) return fail(c, KSCHED_E_STATE, "load_ext before load_nodes");
    if (c->o.nranks > 1) return fail(c, KSCHED_E_INVALID, "load_ext: extended resources are single-GPU (the exact kernel)");
    if (const char *why = ext_check_table(n_ext, node_ext)) return fail(c, KSCHED_E_INVALID, std::string("load_ext: ") + why);
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ext_R = 0;
    const size_t bytes = (size_t)n_ext * (size_t)c->n_local * 8;
    HIPCHK(c, c->d->etab.reserve(bytes));
    if (bytes > 0) HIPCHK(c, hipMemcpyAsync(c->d->etab, node_ext, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's array is free again
    c->ext_R = n_ext;
    return KSCHED_OK;
}

int ksched_read_ext(ksched_ctx *c, int64_t *out_ext) {
    if (!c) return KSCHED_E_INVALID;
    if (c->ext_R == 0) return fail(c, KSCHED_E_STATE, "read_ext: no extended-resource table (ksched_load_ext after every ksched_load_nodes)");
    if (!out_ext) return fail(c, KSCHED_E_INVALID, "read_ext: out_ext is NULL");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t bytes = (size_t)c->ext_R * (size_t)c->n_local * 8;
    if (bytes > 0) HIPCHK(c, hipMemcpy(out_ext, c->d->etab, bytes, hipMemcpyDeviceToHost));
    return KSCHED_OK;
}

// The affinity table of ksched_schedule_affinity: checked on the host (ksched_affinity.h), and its zone and `any` words
// derived there, before anything is allocated or staged; then uploaded in the stream of the kernel that reads it.
// Touches no node row; the context holds the new table only once the last copy has landed, and the earlier one until the
// checks have passed.
int ksched_load_affinity(ksched_ctx *c, int32_t n_domains, const int32_t *node_domain, const uint64_t *node_member,
                         const uint64_t *node_anti_host, const uint64_t *node_anti_zone) {
    if (!c) return KSCHED_E_INVALID;
    static_assert(KSCHED_AFF_MAX_GROUPS == kAffMaxGroups && kAffPodWords == kAffWords, "affinity constants");
    if (c->n_local < 0) return fail(c, KSCHED_E_STATE, "load_affinity before load_nodes");
    if (c->o.nranks > 1) return fail(c, KSCHED_E_INVALID, "load_affinity: affinity scheduling is single-GPU (the exact kernel)");
    AffDerived der;
    try {
        if (const char *why = aff_check_table(c->n_local, n_domains, node_domain))
            return fail(c, KSCHED_E_INVALID, std::string("load_affinity: ") + why);
        aff_derive(c->n_local, n_domains, node_domain, node_member, node_anti_zone, &der);
    } catch (const std::bad_alloc &) {
        return fail(c, KSCHED_E_NOMEM, "load_affinity: host allocation failed");
    }
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->aff_valid = false;
    ksched_bufs &d = *c->d;
    const size_t n = (size_t)c->n_local, zb = der.zone.size() * 8;
    HIPCHK(c, d.adom.reserve(n * 4)); HIPCHK(c, d.amem.reserve(n * 8)); HIPCHK(c, d.aanti_h.reserve(n * 8));
    HIPCHK(c, d.aanti_z.reserve(n * 8)); HIPCHK(c, d.azone.reserve(zb)); HIPCHK(c, d.aany.reserve(16));
    if (n > 0) {
        // (node_domain may be null only where no node carries a zone: every domain -1, all bytes 0xff)
        if (node_domain) HIPCHK(c, hipMemcpyAsync(d.adom, node_domain, n * 4, hipMemcpyHostToDevice, c->stream));
        else HIPCHK(c, hipMemsetAsync(d.adom, 0xff, n * 4, c->stream));
        const std::pair<uint64_t *, const uint64_t *> masks[] = {
            {d.amem.p, node_member}, {d.aanti_h.p, node_anti_host}, {d.aanti_z.p, node_anti_zone}};
        for (const auto &m : masks) {
            if (m.second) HIPCHK(c, hipMemcpyAsync(m.first, m.second, n * 8, hipMemcpyHostToDevice, c->stream));
            else HIPCHK(c, hipMemsetAsync(m.first, 0, n * 8, c->stream));
        }
    }
    if (zb > 0) HIPCHK(c, hipMemcpyAsync(d.azone, der.zone.data(), zb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's arrays, and der, are free again
    c->aff_D = n_domains;
    c->aff_any[0] = der.any_host; c->aff_any[1] = der.any_zone;
    c->aff_valid = true;
    return KSCHED_OK;
}

int ksched_read_affinity(ksched_ctx *c, uint64_t *out_member, uint64_t *out_anti_host, uint64_t *out_anti_zone) {
    if (!c) return KSCHED_E_INVALID;
    if (!c->aff_valid) return fail(c, KSCHED_E_STATE, "read_affinity: no affinity table (ksched_load_affinity after every ksched_load_nodes)");
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t bytes = (size_t)c->n_local * 8;
    if (bytes > 0) {
        if (out_member) HIPCHK(c, hipMemcpy(out_member, c->d->amem, bytes, hipMemcpyDeviceToHost));
        if (out_anti_host) HIPCHK(c, hipMemcpy(out_anti_host, c->d->aanti_h, bytes, hipMemcpyDeviceToHost));
        if (out_anti_zone) HIPCHK(c, hipMemcpy(out_anti_zone, c->d->aanti_z, bytes, hipMemcpyDeviceToHost));
    }
    return KSCHED_OK;
}

// The constrained schedule calls: each names its kind and its arguments (FullArgs: p, the gangs, spread, extended
// resources, the five affinity arrays; what the call has not stays null) and runs through schedule_kind.  In a composed
// call (kRunAll, kRunFull, kRunFullWhy) a constraint whose argument is NULL (affinity: all five) is off for the whole
// call: its per-pod words say so and the kernel is not given its table.
int ksched_schedule_gangs(ksched_ctx *c, int64_t p, const int64_t *rc, const int64_t *rm, const int64_t *rp,
                          const uint64_t *sel, int64_t n_gangs, const int64_t *gang_off, const int32_t *gang_min,
                          int32_t *oi, double *os, int32_t *of, int32_t *out_gang_placed) {
    const FullArgs args{p, n_gangs, gang_off, gang_min};
    return schedule_kind(c, kRunGang, "schedule_gangs", args, PodIO{rc, rm, rp, sel, oi, os, of}, out_gang_placed);
}

int ksched_schedule_spread(ksched_ctx *c, int64_t p, const int64_t *rc, const int64_t *rm, const int64_t *rp,
                           const uint64_t *sel, const int32_t *spread_group, const uint8_t *spread_enforce, int32_t *oi,
                           double *os, int32_t *of) {
    const FullArgs args{p, 0, nullptr, nullptr, spread_group, spread_enforce};
    return schedule_kind(c, kRunSpread, "schedule_spread", args, PodIO{rc, rm, rp, sel, oi, os, of}, nullptr);
}

int ksched_schedule_ext(ksched_ctx *c, int64_t p, const int64_t *rc, const int64_t *rm, const int64_t *rp,
                        const uint64_t *sel, const int64_t *req_ext, int32_t *oi, double *os, int32_t *of) {
    const FullArgs args{p, 0, nullptr, nullptr, nullptr, nullptr, req_ext};
    return schedule_kind(c, kRunExt, "schedule_ext", args, PodIO{rc, rm, rp, sel, oi, os, of}, nullptr);
}

int ksched_schedule_constrained(ksched_ctx *c, int64_t p, const int64_t *rc, const int64_t *rm, const int64_t *rp,
                                const uint64_t *sel, int64_t n_gangs, const int64_t *gang_off, const int32_t *gang_min,
                                const int32_t *spread_group, const uint8_t *spread_enforce, const int64_t *req_ext,
                                int32_t *oi, double *os, int32_t *of, int32_t *out_gang_placed) {
    const FullArgs args{p, n_gangs, gang_off, gang_min, spread_group, spread_enforce, req_ext};
    return schedule_kind(c, kRunAll, "schedule_constrained", args, PodIO{rc, rm, rp, sel, oi, os, of}, out_gang_placed);
}

int ksched_schedule_affinity(ksched_ctx *c, int64_t p, const int64_t *rc, const int64_t *rm, const int64_t *rp,
                             const uint64_t *sel, const uint64_t *member, const uint64_t *anti_host,
                             const uint64_t *anti_zone, const int32_t *aff_group, const uint8_t *aff_zone, int32_t *oi,
                             double *os, int32_t *of) {
    const FullArgs args{p, 0, nullptr, nullptr, nullptr, nullptr, nullptr, member, anti_host, anti_zone, aff_group, aff_zone};
    return schedule_kind(c, kRunAffinity, "schedule_affinity", args, PodIO{rc, rm, rp, sel, oi, os, of}, nullptr);
}

int ksched_schedule_full(ksched_ctx *c, int64_t p, const int64_t *rc, const int64_t *rm, const int64_t *rp,
                         const uint64_t *sel, int64_t n_gangs, const int64_t *gang_off, const int32_t *gang_min,
                         const int32_t *spread_group, const uint8_t *spread_enforce, const int64_t *req_ext,
                         const uint64_t *member, const uint64_t *anti_host, const uint64_t *anti_zone,
                         const int32_t *aff_group, const uint8_t *aff_zone, int32_t *oi, double *os, int32_t *of,
                         int32_t *out_gang_placed) {
    const FullArgs args{p, n_gangs, gang_off, gang_min, spread_group, spread_enforce, req_ext, member, anti_host, anti_zone,
                        aff_group, aff_zone};
    return schedule_kind(c, kRunFull, "schedule_full", args, PodIO{rc, rm, rp, sel, oi, os, of}, out_gang_placed);
}

// ksched_schedule_full, and what every pod that fits nowhere saw at its turn.  The call's own arguments are checked
// behind ksched_schedule_full's (ksched_why.h), and the rows' buffer is reserved and cleared, before anything is staged:
// a refused call and a failed allocation leave the context as it was.
int ksched_schedule_full_why(ksched_ctx *c, int64_t p, const int64_t *rc, const int64_t *rm, const int64_t *rp,
                             const uint64_t *sel, int64_t n_gangs, const int64_t *gang_off, const int32_t *gang_min,
                             const int32_t *spread_group, const uint8_t *spread_enforce, const int64_t *req_ext,
                             const uint64_t *member, const uint64_t *anti_host, const uint64_t *anti_zone,
                             const int32_t *aff_group, const uint8_t *aff_zone, int32_t *oi, double *os, int32_t *of,
                             int32_t *out_gang_placed, int64_t why_rows, int32_t *out_why_pod, int64_t *out_why_counts,
                             int64_t node_rows, uint8_t *out_why_reason, int64_t *out_nofit) {
    const FullArgs args{p, n_gangs, gang_off, gang_min, spread_group, spread_enforce, req_ext, member, anti_host, anti_zone,
                        aff_group, aff_zone};
    FullPacked k;
    if (const int r = constrained_begin(c, kRunFullWhy, "schedule_full_why", args, &k)) return r;
    const int64_t n = c->n_local;
    if (const char *why = why_check(WhyArgs{why_rows, out_why_pod, out_why_counts, node_rows, out_why_reason, n}))
        return fail(c, KSCHED_E_INVALID, std::string("schedule_full_why: ") + why);
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const WhyLayout l = why_layout(why_rows, node_rows, n);
    if (c->d->why.reserve(l.total) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, KSCHED_E_NOMEM, "schedule_full_why: the rows' device buffer");
    }
    // counts, total and bytes 0, every pod -1: a row the kernel does not reach reads as the header words it
    char *w = static_cast<char *>(c->d->why.p);
    HIPCHK(c, hipMemsetAsync(w, 0, l.total, c->stream));
    if (why_rows > 0) HIPCHK(c, hipMemsetAsync(w + l.o_pod, 0xff, (size_t)why_rows * 4, c->stream));
    c->why_rows = why_rows; c->why_node_rows = node_rows;
    const int r = constrained_run(c, kRunFullWhy, "schedule_full_why", args, k, PodIO{rc, rm, rp, sel, oi, os, of}, out_gang_placed);
    if (r != KSCHED_OK) return r;
    // (the run's sync is behind the kernel, or -- no pods, no launch -- behind the clears alone)
    int64_t total = 0;
    HIPCHK(c, hipMemcpy(&total, w + l.o_nofit, 8, hipMemcpyDeviceToHost));
    if (why_rows > 0) {
        HIPCHK(c, hipMemcpy(out_why_pod, w + l.o_pod, (size_t)why_rows * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(out_why_counts, w + l.o_counts, (size_t)why_rows * KSCHED_NUM_REASONS_FULL * 8, hipMemcpyDeviceToHost));
    }
    if (node_rows > 0 && n > 0) HIPCHK(c, hipMemcpy(out_why_reason, w + l.o_reason, (size_t)node_rows * (size_t)n, hipMemcpyDeviceToHost));
    if (out_nofit) *out_nofit = total;
    return KSCHED_OK;
}

// Ranked dry run under constraints (ksched_dryrun.hip).  Touches nothing a schedule call left behind and no table: the
// groups' minima, its pods, span lists and outputs live in d->dws, and FAST53 is decided here for these m pods alone.
int ksched_rank_full(ksched_ctx *c, int64_t m, const int64_t *rc, const int64_t *rm, const int64_t *rp, const uint64_t *sel,
                     const int32_t *spread_group, const uint8_t *spread_enforce, const int64_t *req_ext,
                     const uint64_t *member, const uint64_t *anti_host, const uint64_t *anti_zone, const int32_t *aff_group,
                     const uint8_t *aff_zone, int32_t k, int32_t *out_idx, double *out_score, uint8_t *out_reason,
                     int32_t *out_count, int32_t *out_feasible, int64_t *out_reason_counts) {
    if (!c) return KSCHED_E_INVALID;
    static_assert(KSCHED_NUM_REASONS_FULL == kNumReasonsFull && KSCHED_RANK_MAX == 64, "dry run constants");
    if (k < 1 || k > KSCHED_RANK_MAX) return fail(c, KSCHED_E_INVALID, "rank_full: k must be in 1..KSCHED_RANK_MAX");
    DryPacked pk;
    const DryCall call{m, rc, rm, rp, sel, spread_group, spread_enforce, req_ext, member, anti_host, anti_zone, aff_group, aff_zone};
    if (const int r = dry_begin(c, "rank_full", call, &pk)) return r;
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (m == 0) return KSCHED_OK;
    const int64_t n = c->n_local;
    if (n == 0) {  // no node: nothing is ranked and nothing is counted
        const size_t e = (size_t)m * (size_t)k;
        if (out_idx) std::fill(out_idx, out_idx + e, -1);
        if (out_score) std::fill(out_score, out_score + e, 0.0);
        if (out_reason) std::memset(out_reason, 0, e);
        if (out_count) std::fill(out_count, out_count + m, 0);
        if (out_feasible) std::fill(out_feasible, out_feasible + m, 0);
        if (out_reason_counts) std::fill(out_reason_counts, out_reason_counts + m * KSCHED_NUM_REASONS_FULL, (int64_t)0);
        return KSCHED_OK;
    }
    uint64_t mxr = 0;
    for (int64_t i = 0; i < m; ++i) mxr = std::max(mxr, std::max(uabs64(rc[i]), std::max(uabs64(rm[i]), uabs64(rp[i]))));
    const bool f53 = sat_add(c->max_abs_alloc, mxr) < (1ull << 52);
    // the workspace: minima | one chunk's pods | span lists | span histograms | outputs, each 256-byte aligned
    const int64_t mc_max = std::min<int64_t>(m, kRankChunk);
    size_t nl = 0;  // span lists of the largest chunk: at most kRankGridWGs * kDryTile (dry_geometry)
    for (int64_t q : {mc_max, m % kRankChunk}) {  // the full chunk and the tail (fewer pods, more spans)
        if (q <= 0) continue;
        int32_t s; int64_t rows;
        dry_geometry(n, q, &s, &rows);
        nl = std::max(nl, (size_t)q * (size_t)s);
    }
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t o_min = 0, o_pods = al(o_min + KSCHED_SPREAD_MAX_GROUPS * 4), o_part = al(o_pods + (size_t)mc_max * sizeof(DryPod)),
                 o_ph = al(o_part + nl * 64 * sizeof(Cand)), o_idx = al(o_ph + nl * kDryHist * 4),
                 o_sc = al(o_idx + (size_t)mc_max * k * 4), o_rs = al(o_sc + (size_t)mc_max * k * 8),
                 o_cnt = al(o_rs + (size_t)mc_max * k), o_feas = al(o_cnt + (size_t)mc_max * 4),
                 o_hist = al(o_feas + (size_t)mc_max * 4), total = al(o_hist + (size_t)mc_max * kNumReasonsFull * 8);
    HIPCHK(c, c->d->dws.reserve(total));
    char *w = static_cast<char *>(c->d->dws.p);
    const DryTables t = dry_tables(c, pk, reinterpret_cast<int32_t *>(w + o_min));
    HIPCHK(c, launch_dry_min(t, c->stream));
    std::vector<char> stage(total - o_idx);  // host side of a chunk's copy out
    for (int64_t at = 0; at < m; at += kRankChunk) {
        const int64_t mc = std::min<int64_t>(kRankChunk, m - at);
        DryArgs a{};
        a.nodes = c->d->nodes; a.n_local = n; a.node_offset = c->o.node_offset;
        a.t = t;
        a.pods = reinterpret_cast<DryPod *>(w + o_pods);
        a.m = (int32_t)mc; a.k = k;
        dry_geometry(n, mc, &a.spans, &a.span_rows);
        if ((size_t)mc * a.spans > nl) return fail(c, KSCHED_E_NOMEM, "rank_full: workspace bound");  // (dry_geometry's bound)
        a.part = reinterpret_cast<Cand *>(w + o_part); a.part_hist = reinterpret_cast<int32_t *>(w + o_ph);
        a.out_idx = reinterpret_cast<int32_t *>(w + o_idx); a.out_score = reinterpret_cast<double *>(w + o_sc);
        a.out_reason = reinterpret_cast<uint8_t *>(w + o_rs); a.out_count = reinterpret_cast<int32_t *>(w + o_cnt);
        a.out_feasible = reinterpret_cast<int32_t *>(w + o_feas); a.out_hist = reinterpret_cast<int64_t *>(w + o_hist);
        // one copy in and one copy out per chunk, in the stream of the kernels
        HIPCHK(c, hipMemcpyAsync(w + o_pods, pk.pods.data() + at, (size_t)mc * sizeof(DryPod), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_dry_rank(c->o.priority, c->o.domain, c->o.use_labels != 0, f53, a, c->stream));
        HIPCHK(c, hipMemcpyAsync(stage.data(), w + o_idx, total - o_idx, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // the next chunk reuses the workspace and the staging buffer
        const size_t e = (size_t)mc * k, eo = (size_t)at * k;
        const char *ho = stage.data();  // the outputs, at their workspace offsets less o_idx
        if (out_idx) std::memcpy(out_idx + eo, ho, e * 4);
        if (out_score) std::memcpy(out_score + eo, ho + (o_sc - o_idx), e * 8);
        if (out_reason) std::memcpy(out_reason + eo, ho + (o_rs - o_idx), e);
        if (out_count) std::memcpy(out_count + at, ho + (o_cnt - o_idx), (size_t)mc * 4);
        if (out_feasible) std::memcpy(out_feasible + at, ho + (o_feas - o_idx), (size_t)mc * 4);
        if (out_reason_counts)
            std::memcpy(out_reason_counts + at * kNumReasonsFull, ho + (o_hist - o_idx), (size_t)mc * kNumReasonsFull * 8);
    }
    return KSCHED_OK;
}

// One pod's per-node reasons and their histogram under constraints: k_dry_explain behind k_dry_min, in d->dws.
int ksched_explain_full(ksched_ctx *c, int64_t rc, int64_t rm, int64_t rp, uint64_t sel, int32_t spread_group,
                        int32_t spread_enforce, const int64_t *req_ext, uint64_t member, uint64_t anti_host,
                        uint64_t anti_zone, int32_t aff_group, int32_t aff_zone, int64_t out_counts[KSCHED_NUM_REASONS_FULL],
                        uint8_t *out_reason) {
    if (!c) return KSCHED_E_INVALID;
    if (c->n_local < 0) return fail(c, KSCHED_E_STATE, "explain_full before load_nodes");
    if (!out_counts) return fail(c, KSCHED_E_INVALID, "explain_full: out_counts is NULL");
    if (const char *why = dry_check_one(spread_group, aff_group)) return fail(c, KSCHED_E_INVALID, std::string("explain_full: ") + why);
    const DryOne one{rc, rm, rp, sel, member, anti_host, anti_zone, spread_group, aff_group,
                     (uint8_t)(spread_enforce != 0), (uint8_t)(aff_zone != 0)};
    DryPacked pk;
    if (const int r = dry_begin(c, "explain_full", one.call(req_ext), &pk)) return r;
    HIPCHK(c, hipSetDevice(c->dev));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t n = c->n_local;
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t o_min = 0, o_cnt = al(o_min + KSCHED_SPREAD_MAX_GROUPS * 4), o_rs = al(o_cnt + kNumReasonsFull * 8),
                 total = al(o_rs + (size_t)n);
    HIPCHK(c, c->d->dws.reserve(total));
    char *w = static_cast<char *>(c->d->dws.p);
    const DryTables t = dry_tables(c, pk, reinterpret_cast<int32_t *>(w + o_min));
    unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(w + o_cnt);
    unsigned long long h[kNumReasonsFull] = {};
    HIPCHK(c, hipMemsetAsync(d_cnt, 0, sizeof(h), c->stream));
    HIPCHK(c, launch_dry_min(t, c->stream));
    HIPCHK(c, launch_dry_explain(c->d->nodes, n, t, pk.pods[0], c->o.use_labels != 0,
                                 out_reason ? reinterpret_cast<uint8_t *>(w + o_rs) : nullptr, d_cnt, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h, d_cnt, sizeof(h), hipMemcpyDeviceToHost));
    if (out_reason && n > 0) HIPCHK(c, hipMemcpy(out_reason, w + o_rs, (size_t)n, hipMemcpyDeviceToHost));
    for (int r = 0; r < kNumReasonsFull; ++r) out_counts[r] = (int64_t)h[r];
    return KSCHED_OK;
}

}  // extern "C"

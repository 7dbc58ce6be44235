// ksched_exact.hip -- CDNA4 (gfx950) kernels of exact mode: k_exact in the kinds of ksched_exact.h's table (exact_kind),
// the one-workgroup k_exact1, and their launchers.
// Compiled with -ffp-contract=off: every double op rounds individually, exactly like the Go reference.
// Four objects, as ksched_pipe.hip's three (-DKSCHED_EXACT_PART): part 0 is the kinds kRunPlain to kRunAll, k_exact1
// and the launchers; parts 1, 2 and 3 are the 40 instantiations each of kRunAffinity, kRunFull and kRunFullWhy, behind
// launch_exact_affinity, launch_exact_full and launch_exact_full_why.
#include <hip/hip_runtime.h>

#include <mutex>
#include <set>
#include <type_traits>
#include <utility>

#include "ksched_exact.h"
#include "ksched_kernels.h"  // KSCHED_DISPATCH, kErrExactExchange
#include "ksched_reason.h"   // PodU, RowX, dry_reason: k_exact<kRunFullWhy>

#ifndef KSCHED_EXACT_PART
#define KSCHED_EXACT_PART 0
#endif

namespace ksched {

hipError_t launch_exact_affinity(int npt, int prio, int dom, bool lab, bool f53, const ExactArgs &a, int block, bool coop,
                                 hipStream_t s);  // part 1
hipError_t launch_exact_full(int npt, int prio, int dom, bool lab, bool f53, const ExactArgs &a, int block, bool coop,
                             hipStream_t s);  // part 2
hipError_t launch_exact_full_why(int npt, int prio, int dom, bool lab, bool f53, const ExactArgs &a, int block, bool coop,
                                 hipStream_t s);  // part 3

namespace {

__device__ __forceinline__ uint64_t ld_granule(const uint64_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_granule(uint64_t *p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

// k_exact<GANG>: what a workgroup keeps across the pods of the current gang, and its LDS log of their outcomes
struct GangNone {};
struct GangState {
    int64_t gang = 0;             // the current gang,
    int32_t gm = 0, placed = 0;   // ... the current member, the members placed so far
};
template <bool GANG>
__device__ __forceinline__ int32_t *gang_log() {
    if constexpr (GANG) {
        __shared__ int32_t s_log[kGangMax];  // member by member: the node, or the member's failure code
        return s_log;
    } else {
        return nullptr;
    }
}

// k_exact<SPREAD>: a workgroup's copy of the spread table -- the S x D counts row-major, and per group the row's
// minimum, the number of domains at it, and the maximum skew
struct SpreadTable {
    int32_t cnt[kSpreadMaxCells];
    int32_t mn[kSpreadMaxGroups], nmin[kSpreadMaxGroups], skew[kSpreadMaxGroups];
};
template <bool SPREAD>
__device__ __forceinline__ SpreadTable *spread_table() {
    if constexpr (SPREAD) {
        __shared__ SpreadTable s_spread;
        return &s_spread;
    } else {
        return nullptr;
    }
}

// k_exact<EXT>: a workgroup's slots of the extended-resource table, in dynamic LDS: column r of slot s at
// [r * kExactBlock * NPT + s].  (Declared 16-byte aligned: the dynamic region follows the kernel's statics.)
template <bool EXT>
__device__ __forceinline__ int64_t *ext_table() {
    if constexpr (EXT) {
        extern __shared__ __attribute__((aligned(16))) int64_t s_ext[];
        return s_ext;
    } else {
        return nullptr;
    }
}

// k_exact<kRunAll>: the topology domains of a workgroup's slots, slot s = tid + k * kExactBlock at [s] (consecutive
// lanes read consecutive words: conflict-free).  The registers of the spread kernels are full,
// and this kind carries the gang state and the extended-resource pointers beside them.
template <bool ALL, int NPT>
__device__ __forceinline__ int32_t *dom_table() {
    if constexpr (ALL) {
        __shared__ int32_t s_dom[kExactBlock * NPT];
        return s_dom;
    } else {
        return nullptr;
    }
}

// k_exact<AFF>: a workgroup's copy of the zone words of the affinity table, per domain {zone_member, zone_anti} side
// by side (one 16-byte gather per slot), 16 KiB
struct AffZone {
    uint64_t member, anti;
};
template <bool AFF>
__device__ __forceinline__ AffZone *aff_zone() {
    if constexpr (AFF) {
        __shared__ __attribute__((aligned(16))) AffZone s_zone[kSpreadMaxDomains];
        return s_zone;
    } else {
        return nullptr;
    }
}

// k_exact<AFF>: the per-slot words of a workgroup, in dynamic LDS: node_member of slot s = tid + k * kExactBlock at
// [s], node_anti_host at [kExactBlock * NPT + s], and behind them the slots' domains (int32, laid out as dom_table is).
// Consecutive lanes read consecutive words; only the owning thread ever touches a slot's words.
template <bool AFF>
__device__ __forceinline__ uint64_t *aff_table() {
    if constexpr (AFF) {
        extern __shared__ __attribute__((aligned(16))) uint64_t s_aff[];
        return s_aff;
    } else {
        return nullptr;
    }
}

// ------------------------------------------------------------------------------------------------
// Exact mode: one persistent launch schedules every pod in order.
//   - workgroup g owns nodes [g*per_wg, (g+1)*per_wg); thread t holds nodes g*per_wg + t + k*256
//     (k < NPT) in registers for the whole launch, with their (double) values and reciprocals;
//   - per pod: each lane scores its nodes (predicate.go:127-150 + priorities.go:45-50), wave
//     butterfly arg-best + count, 4-wave combine through LDS;
//   - G > 1: wave 0 publishes the workgroup's (key, idx, count) as four tagged 8-byte granules
//     (write-through sc1 stores, epoch = pod + 1) and sweeps all G records until every tag matches
//     (MI355X_MICROARCH "handoff-1to1"/"allgather" R2 granules: no fences needed); every workgroup
//     then folds the same G records into the same decision;
//   - the owner lane of the winning node commits it in registers; nodes are written back at exit.
// GANG (ksched_schedule_gangs): the pods come in groups that are bound all-or-nothing.
//   Every member is evaluated and committed exactly as above -- never skipped, so the granule tag and the parity
//   advance by one per pod -- and every workgroup logs the member's outcome in LDS (s_log, thread 0: the decision
//   is the same in every thread of every workgroup).  At the gang's last member every workgroup compares the
//   same count of placed members with the gang's minimum.  Rejected: one workgroup barrier (the log's last
//   entry), then every thread walks the log and adds the members' requests back to the slots it owns (wrapping,
//   the commit's inverse; f / y re-derived once per touched slot), and workgroup 0 rewrites the placed members'
//   results.  Register-only and workgroup-local: no exchange, no wait.  The next gang's first log entry is
//   written behind the next pod's barrier, after every thread has left the walk.
// SPREAD (ksched_schedule_spread): one topology spread constraint per pod joins the
//   predicate.  Every thread keeps its slots' domains in registers; every workgroup keeps the whole S x D count
//   table in LDS (SpreadTable, loaded at entry, written back by workgroup 0 at exit) with each row's minimum and
//   the number of domains at it.  An enforcing pod's slot is eligible when it fits and counts[s][dom] <= skew[s] +
//   min[s] - 1: one LDS gather per slot and two broadcast reads per pod.  Every workgroup derives the same winner,
//   reads its domain from the global array (a uniform load) and thread 0 applies the same increment to its own
//   copy -- no exchange, no wait, the tag and parity sequence unchanged.  A row's minimum rises only when its last
//   domain at the minimum is incremented; thread 0 then recounts the row (D reads, at most once per D placements
//   of the group).  The increment is written after the pod's last barrier and the next pod's gathers come before
//   its first, so a pod that moved the table ends with one more barrier; a pod that did not (no group, not placed,
//   a node without the key) pays none.
// EXT (ksched_schedule_ext): up to kExtMax further resource columns join the predicate.  The
//   registers are full (section 4.7), so the columns of a workgroup's slots live in dynamic LDS, ext[r][slot] with
//   slot = tid + k * kExactBlock: consecutive lanes read consecutive 8-byte words.  Loaded from the device table at
//   entry (node ids below n only), written back by every workgroup for its own slots at exit.  The pod's requests
//   come pod-major with a word of non-zero-column bits, all uniform loads: a column the pod does not ask for is a
//   uniform skip, so a pod that asks for nothing reads no LDS.  The owner lane of the winning slot subtracts the
//   non-zero requests from its own slot's words.  Only the owning thread ever reads or writes a slot's words: no
//   new barrier, exchange or wait; the tag and parity sequence unchanged.
// ALL (ksched_schedule_constrained): the three together, the only pairing instantiated.  A
//   constraint the call does not use is switched off by uniform runtime values: sp_S == 0 (no table is loaded or
//   written back, every sp_word is -1), n_ext == 0 (no dynamic LDS, every ext_word is 0), gangs of one.  The slots'
//   domains live in LDS (dom_table), not in registers.  A rejected gang's walk over the log also undoes the other two
//   commits: the owner lane of a logged member's slot adds the member's non-zero requests back to its own words
//   (ext_word / ext_req reloaded, uniform, as the cpu and memory requests are), and thread 0 of every workgroup
//   decrements the count of every logged member with a group on a node that carries the key, keeping the row's
//   minimum and the number of domains at it exact per decrement (a value below the minimum becomes the minimum, held
//   once; a value equal to it is one more holder).  The next pod's gathers read the table before its first barrier, so
//   a walk that moved the table ends with one barrier (workgroup-uniform: rejected, and a logged member was counted).
// AFF (ksched_schedule_affinity): required inter-pod affinity and anti-affinity over at most 64
//   selector groups, one bit of a 64-bit word each, at host scope (every node its own domain) and zone scope (af_dom).
//   Paired with no other kind.  The slots' node_member and node_anti_host words and their domains live in dynamic LDS
//   (aff_table; the registers are full), touched by the owning thread only; every workgroup keeps the whole zone table
//   {zone_member, zone_anti}[D] in static LDS (AffZone, loaded at entry, written back by workgroup 0 at exit); any_host
//   and any_zone are workgroup-uniform values that every thread carries.  The pod's four words come with its request as
//   uniform loads, behind a staged word that is 0 for a pod without group or term: such a pod reads no LDS and commits
//   nothing.  A slot is eligible when it fits and three AND tests of the pod's words against the slot's and its zone's
//   words pass (include/ksched.h).  Every workgroup derives the same winner; its owner lane ORs the pod's words into its
//   own slot's words (node_anti_zone, which no test reads, straight into the global array), every thread ORs member into
//   its any words, and thread 0 ORs into its workgroup's zone words behind a uniform load of the winner's domain -- no
//   exchange, no wait, the tag and parity sequence unchanged.  The next pod's gathers read the zone table before its
//   first barrier, so a pod that may have moved it ends with one barrier; its condition -- placed, the winner's domain
//   >= 0, (member | anti_zone) != 0 -- is made of uniform inputs only, never of the LDS words thread 0 is writing.
// FULL (ksched_schedule_full): ALL and AFF together.  Affinity too is switched off by a uniform
//   runtime value (af_dom null: no table is loaded or written back, no affinity slot words in LDS, every af_word is 0);
//   the affinity slot words lie behind the n_ext columns of the dynamic region.  The affinity words only gain bits, so a
//   rejected gang restores old values from a log in device memory (the LDS is full): at a logging member's commit the
//   winner's owner lane writes its slot's node_member, node_anti_host and -- where it is about to OR into it --
//   node_anti_zone to af_undo_slot[member], and thread 0 of every workgroup writes its copy of the winner's zone words to
//   af_undo_zone[workgroup][member], both BEFORE the OR; every thread keeps the any words of the gang's first member in
//   registers.  A gang of one never rolls a commit back and logs nothing.  The walk runs newest member first, so a slot
//   or zone hit several times ends at its oldest logged value; every thread reads back only what it wrote itself (same
//   thread, same address: program order, no fence).  The walk's closing barrier gains one more workgroup-uniform reason:
//   a logged member moved a zone word (its af_word, its words and its winner's domain: uniform loads from arrays nobody
//   writes).  No exchange, no wait, the tag and parity sequence unchanged.
// WHY (ksched_schedule_full_why): FULL, and where the decision is NO_FIT -- the same in every
//   thread of every workgroup, so a pod that finds a node pays one uniform branch -- every thread gives each slot it owns
//   its reason code at this pod's turn: dry_reason (ksched_reason.h), the function the dry runs explain with, over the
//   row registers, the columns, domains and words in LDS and the pod's words after the waiver.  The state is the one a
//   rollback would erase: the tentative commits of the earlier members of the pod's own gang are in it.  The codes go to
//   why_reason (a byte per node, consecutive lanes consecutive bytes) and, summed per wave in packed fields, to the
//   pod's row of why_counts with one device-scope integer atomicAdd per wave for the codes that occur (integer sums: any
//   order).  Every thread counts the NO_FIT pods in a scalar; a rollback never touches it.  Nothing here feeds a
//   decision: no new LDS, barrier, exchange or wait, the tag and parity sequence unchanged.
// ------------------------------------------------------------------------------------------------
template <int NPT, int PRIO, int DOM, bool LAB, bool F53, ExactRun RUN>
__global__ __launch_bounds__(kExactBlock) void k_exact(ExactArgs A) {
    constexpr ExactKind KIND = exact_kind(RUN);
    constexpr bool WHY = KIND.why, FULL = KIND.undo, ALL = KIND.optional, AFF = KIND.aff;
    constexpr bool GANG = KIND.gang, SPREAD = KIND.spread, EXT = KIND.ext;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int g = blockIdx.x;
    const int64_t lo = (int64_t)g * A.per_wg;
    const int64_t hi = (lo + A.per_wg < A.n) ? lo + A.per_wg : A.n;
    const double y3 = recip(3.0);

    int64_t a0[NPT], a1[NPT], a2[NPT];
    double f0[NPT], f1[NPT], f2[NPT], y0[NPT], y1[NPT], y2[NPT];
    uint64_t lab[NPT];
    float pr[NPT];
    int32_t id[NPT];
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const int64_t j = lo + tid + (int64_t)k * kExactBlock;
        if (j < hi) {
            const NodeRec &nd = A.nodes[j];
            a0[k] = nd.a[0]; a1[k] = nd.a[1]; a2[k] = nd.a[2];
            f0[k] = nd.af[0]; f1[k] = nd.af[1]; f2[k] = nd.af[2];
            y0[k] = nd.y[0]; y1[k] = nd.y[1]; y2[k] = nd.y[2];
            lab[k] = nd.labels; pr[k] = nd.price; id[k] = (int32_t)j;
        } else {
            a0[k] = a1[k] = a2[k] = 0; f0[k] = f1[k] = f2[k] = 0.0; y0[k] = y1[k] = y2[k] = 0.0;
            lab[k] = 0; pr[k] = 0.f; id[k] = kNoIdx;
        }
    }
    // SPREAD: the slots' topology domains (-1: the node lacks the key).  ALL: the same in LDS, this thread's slot k at
    // s_dom[k * kExactBlock] (no other thread touches it); every one -1 where sp_S == 0 says there is no table
    [[maybe_unused]] int32_t dom[SPREAD && !ALL ? NPT : 1];
    [[maybe_unused]] int32_t *const s_dom = ALL ? dom_table<ALL, NPT>() + tid : nullptr;
    [[maybe_unused]] SpreadTable *const sp = spread_table<SPREAD>();
    if constexpr (SPREAD) {
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            if constexpr (ALL) s_dom[k * kExactBlock] = A.sp_S > 0 && id[k] != kNoIdx ? A.sp_dom[id[k]] : -1;
            else dom[k] = id[k] != kNoIdx ? A.sp_dom[id[k]] : -1;
        }
        const int cells = A.sp_S * A.sp_D;
        for (int c = tid; c < cells; c += kExactBlock) sp->cnt[c] = A.sp_counts[c];
        __syncthreads();
        if (tid < A.sp_S) {  // one thread per group: the row's minimum and how many domains hold it
            const int32_t *row = sp->cnt + tid * A.sp_D;
            int32_t m = row[0], nm = 1;
            for (int d = 1; d < A.sp_D; ++d) {
                const int32_t v = row[d];
                nm = v < m ? 1 : nm + (v == m);
                m = v < m ? v : m;
            }
            sp->mn[tid] = m; sp->nmin[tid] = nm; sp->skew[tid] = A.sp_skew[tid];
        }
        __syncthreads();
    }
    // EXT: this thread's words of column r, slot k at ext[r * kExtCol + k * kExactBlock] (no other thread touches them)
    [[maybe_unused]] constexpr int kExtCol = kExactBlock * NPT;
    [[maybe_unused]] int64_t *const ext = EXT ? ext_table<EXT>() + tid : nullptr;
    if constexpr (EXT) {
        for (int r = 0; r < A.n_ext; ++r) {
#pragma unroll
            for (int k = 0; k < NPT; ++k)
                ext[r * kExtCol + k * kExactBlock] = id[k] != kNoIdx ? A.ext[(int64_t)r * A.n + id[k]] : 0;
        }
    }
    // AFF: this thread's slot k: node_member at af_mem[k * kExactBlock], node_anti_host at af_anti[k * kExactBlock], the
    // domain at af_dom[k * kExactBlock] (no other thread touches them); the zone table; the any words
    // FULL: behind the n_ext columns of the dynamic region; af_on false (no table): nothing is loaded, and no pod reads it
    [[maybe_unused]] const bool af_on = FULL ? A.af_dom != nullptr : AFF;
    [[maybe_unused]] uint64_t *const af_base = AFF ? aff_table<AFF>() + (FULL ? A.n_ext * (kExactBlock * NPT) : 0) : nullptr;
    [[maybe_unused]] uint64_t *const af_mem = AFF ? af_base + tid : nullptr;
    [[maybe_unused]] uint64_t *const af_anti = AFF ? af_mem + kExactBlock * NPT : nullptr;
    [[maybe_unused]] int32_t *const af_dom = AFF ? (int32_t *)(af_base + 2 * kExactBlock * NPT) + tid : nullptr;
    [[maybe_unused]] AffZone *const zone = aff_zone<AFF>();
    [[maybe_unused]] uint64_t any_host = AFF ? A.af_any_host : 0, any_zone = AFF ? A.af_any_zone : 0;
    [[maybe_unused]] uint64_t sv_host = 0, sv_zone = 0;  // FULL: the any words before the current gang's first member
    if constexpr (AFF) {
        if (af_on) {  // (uniform)
#pragma unroll
            for (int k = 0; k < NPT; ++k) {
                const bool own = id[k] != kNoIdx;
                af_mem[k * kExactBlock] = own ? A.af_member[id[k]] : 0;
                af_anti[k * kExactBlock] = own ? A.af_anti_host[id[k]] : 0;
                af_dom[k * kExactBlock] = own ? A.af_dom[id[k]] : -1;
            }
            for (int d = tid; d < A.af_D; d += kExactBlock) {
                zone[d].member = A.af_zone[2 * d];
                zone[d].anti = A.af_zone[2 * d + 1];
            }
            __syncthreads();
        }
    }

    __shared__ double s_key[2][kExactBlock / 64];
    __shared__ int32_t s_idx[2][kExactBlock / 64];
    __shared__ int64_t s_cnt[2][kExactBlock / 64];
    __shared__ double s_rkey[2];
    __shared__ int32_t s_ridx[2];
    __shared__ int64_t s_rcnt[2];
    __shared__ int32_t s_abort;
    if (tid == 0) s_abort = 0;
    [[maybe_unused]] std::conditional_t<GANG, GangState, GangNone> gs;  // (nothing in the plain kernels)
    [[maybe_unused]] int32_t *const s_log = gang_log<GANG>();
    [[maybe_unused]] int64_t nofit = 0;  // WHY: the NO_FIT pods so far, the same in every thread; never rolled back

    for (int64_t i = 0; i < A.pods.p; ++i) {
        const int par = (int)(i & 1);
        const int64_t rc = A.pods.rc[i], rm = A.pods.rm[i], rp = A.pods.rp[i];
        const uint64_t sel = LAB ? A.pods.sel[i] : 0;
        // GANG: 0, or at a gang's last member its size | minimum << 16 -- loaded with the request, not after the pod
        const int32_t gend = GANG ? A.gang_end[i] : 0;
        // SPREAD: -1 (no group), or group << 1 | enforce -- loaded with the request too
        [[maybe_unused]] const int32_t sword = SPREAD ? A.sp_word[i] : -1;
        [[maybe_unused]] bool enf = false;   // the pod enforces its group's constraint:
        [[maybe_unused]] int32_t srow = 0;   // ... the group's row of the table,
        [[maybe_unused]] int64_t slim = 0;   // ... the largest count an eligible domain may hold
        if constexpr (SPREAD) {
            if (sword >= 0 && (sword & 1)) {
                const int32_t s = sword >> 1;
                enf = true;
                srow = s * A.sp_D;
                slim = (int64_t)sp->skew[s] + sp->mn[s] - 1;
            }
        }
        // EXT: the non-zero-column bits -- loaded with the request too -- and, only where there are any, the requests
        // (pod-major: one uniform load; loading them for every pod cost 4 % per pod on pods that ask for nothing)
        [[maybe_unused]] const int32_t eword = EXT ? A.ext_word[i] : 0;
        [[maybe_unused]] int64_t er[EXT ? kExtMax : 1];
        if constexpr (EXT) {
#pragma unroll
            for (int r = 0; r < kExtMax; ++r) er[r] = 0;
            if (eword != 0) {
#pragma unroll
                for (int r = 0; r < kExtMax; ++r) er[r] = A.ext_req[i * kExtMax + r];
            }
        }
        // AFF: 0 (no group, no term: nothing is read or committed), or 1 | zone scope << 1 -- loaded with the request
        // too -- and, only where it is set, the pod's words (pod-major: uniform loads)
        [[maybe_unused]] const int32_t aword = AFF ? A.af_word[i] : 0;
        [[maybe_unused]] uint64_t pmem = 0, pah = 0, paz = 0, pabit = 0;
        [[maybe_unused]] bool azone = false;  // the affinity term (pabit != 0) is of zone scope
        // FULL: this member's commits go to the undo log -- not in a gang of one, which never rolls a commit back
        [[maybe_unused]] bool logit = false;
        if constexpr (FULL) {
            logit = gs.gm != 0 || gend == 0;
            if (gs.gm == 0) { sv_host = any_host; sv_zone = any_zone; }
        }
        if constexpr (AFF) {
            if (aword != 0) {
                pmem = A.af_pod[i * kAffWords]; pah = A.af_pod[i * kAffWords + 1];
                paz = A.af_pod[i * kAffWords + 2]; pabit = A.af_pod[i * kAffWords + 3];
                azone = (aword & 2) != 0;
                // waived: no pod of the group is bound anywhere in scope and the pod is in the group itself
                if ((pabit & (azone ? any_zone : any_host)) == 0 && (pabit & pmem) != 0) pabit = 0;
            }
        }
        const double rcf = (double)rc, rmf = (double)rm, rpf = (double)rp;
        double bk = -__builtin_inf();
        int32_t bi = kNoIdx;
        int64_t cnt = 0;
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            if (id[k] != kNoIdx) {
                bool f = fits(rc, rm, rp, sel, a0[k], a1[k], a2[k], lab[k], LAB);
                if constexpr (SPREAD) {
                    if constexpr (ALL) {
                        if (enf) {
                            const int32_t dk = s_dom[k * kExactBlock];
                            f = f && dk >= 0 && (int64_t)sp->cnt[srow + (dk < 0 ? 0 : dk)] <= slim;
                        }
                    } else {
                        if (enf) f = f && dom[k] >= 0 && (int64_t)sp->cnt[srow + (dom[k] < 0 ? 0 : dom[k])] <= slim;
                    }
                }
                if constexpr (EXT) {
                    if (eword != 0) {  // (uniform: a pod that asks for no column reads no LDS)
#pragma unroll
                        for (int r = 0; r < kExtMax; ++r)
                            if (eword >> r & 1) f = f && er[r] <= ext[r * kExtCol + k * kExactBlock];
                    }
                }
                if constexpr (AFF) {
                    if (aword != 0) {  // (uniform: a pod without group or term reads no LDS)
                        const uint64_t nm = af_mem[k * kExactBlock], na = af_anti[k * kExactBlock];
                        const int32_t dk = af_dom[k * kExactBlock];
                        // own anti-affinity | the bound pods' anti-affinity, host scope; then the same at zone scope,
                        // which a node without the key cannot violate
                        uint64_t bad = (nm & pah) | (na & pmem);
                        uint64_t zm = 0;
                        if (dk >= 0) {
                            const AffZone z = zone[dk];
                            bad |= (z.member & paz) | (z.anti & pmem);
                            zm = z.member;
                        }
                        // own affinity (pabit == 0: none, or waived): the group on this node, or in its zone
                        f = f && bad == 0 && ((azone ? zm : nm) & pabit) == pabit;
                    }
                }
                cnt += f;
                double key;
                if (pair_key_fast<PRIO, DOM, F53>(f, rc, rm, rp, rcf, rmf, rpf, a0[k], a1[k], a2[k], f0[k], f1[k],
                                                  f2[k], y0[k], y1[k], y2[k], y3, pr[k], &key) &&
                    better(key, id[k], bk, bi)) {
                    bk = key;
                    bi = id[k];
                }
            }
        }
        int32_t aux = 0;
        wave_argbest(bk, bi, aux);
        cnt = wave_sum_i64(cnt);
        if (lane == 0) { s_key[par][wave] = bk; s_idx[par][wave] = bi; s_cnt[par][wave] = cnt; }
        __syncthreads();
        double gk = s_key[par][0];
        int32_t gi = s_idx[par][0];
        int64_t gc = s_cnt[par][0];
#pragma unroll
        for (int w = 1; w < kExactBlock / 64; ++w) {
            gc += s_cnt[par][w];
            if (better(s_key[par][w], s_idx[par][w], gk, gi)) { gk = s_key[par][w]; gi = s_idx[par][w]; }
        }
        if (A.G > 1) {
            if (wave == 0) {
                const uint64_t ep = (uint64_t)(uint32_t)(i + 1) << 32;
                uint64_t *mine = A.slots + ((size_t)par * A.G + g) * 4;
                const uint64_t kb = (uint64_t)__double_as_longlong(gk);
                if (lane < 4) {
                    const uint32_t v = lane == 0 ? (uint32_t)(kb >> 32)
                                     : lane == 1 ? (uint32_t)kb
                                     : lane == 2 ? (uint32_t)gi
                                                 : (uint32_t)gc;
                    st_granule(mine + lane, ep | v);
                }
                const int64_t t0 = wall_clock64();
                double fk;
                int32_t fi;
                int64_t fc;
                for (;;) {
                    bool ok = true;
                    fk = -__builtin_inf(); fi = kNoIdx; fc = 0;
                    for (int g2 = lane; g2 < A.G; g2 += 64) {
                        const uint64_t *sl = A.slots + ((size_t)par * A.G + g2) * 4;
                        const uint64_t x0 = ld_granule(sl), x1 = ld_granule(sl + 1);
                        const uint64_t x2 = ld_granule(sl + 2), x3 = ld_granule(sl + 3);
                        ok &= ((x0 & 0xffffffff00000000ull) == ep) & ((x1 & 0xffffffff00000000ull) == ep) &
                              ((x2 & 0xffffffff00000000ull) == ep) & ((x3 & 0xffffffff00000000ull) == ep);
                        const double k2 = __longlong_as_double((long long)((x0 << 32) | (x1 & 0xffffffffull)));
                        const int32_t i2 = (int32_t)(uint32_t)x2;
                        fc += (int64_t)(uint32_t)x3;
                        if (better(k2, i2, fk, fi)) { fk = k2; fi = i2; }
                    }
                    if (__all(ok)) break;
                    if (wall_clock64() - t0 > A.timeout_ticks) {
                        if (lane == 0) { atomicExch(A.err, kErrExactExchange); s_abort = 1; }
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                int32_t aux2 = 0;
                wave_argbest(fk, fi, aux2);
                fc = wave_sum_i64(fc);
                if (lane == 0) { s_rkey[par] = fk; s_ridx[par] = fi; s_rcnt[par] = fc; }
            }
            __syncthreads();
            if (s_abort) break;
            gk = s_rkey[par]; gi = s_ridx[par]; gc = s_rcnt[par];
        }
        int32_t oidx;
        double osc = 0.0;
        if (gc == 0) {
            oidx = -1;  // NO_FIT (anchor/schedule.go:74-76)
            if constexpr (WHY) {
                // the reasons this pod saw: the rows, columns and words exactly as its scan above read them -- nothing
                // has been committed since, and the next writer of either table (thread 0, at a later pod's commit or
                // behind the first barrier of this gang's walk) comes after a barrier that this thread reaches only
                // once it is through here.  Nothing below feeds a decision.
                const int64_t row = nofit++;
                if (__builtin_expect(row < A.why_rows, 0)) {  // (uniform, and rare beside the pods that find a node)
                    PodU u;
                    u.rc = rc; u.rm = rm; u.rp = rp; u.sel = sel;
                    u.mem = pmem; u.anti_h = pah; u.anti_z = paz; u.abit = pabit;  // (pabit: after the waiver)
#pragma unroll
                    for (int r = 0; r < kExtMax; ++r) u.er[r] = er[r];
                    u.srow = enf ? srow : -1; u.slim = slim;
                    u.flags = aword != 0 ? kDryAff | (azone ? kDryAffZone : 0) : 0;
                    const bool bytes = row < A.why_node_rows;
                    uint64_t h0 = 0, h1 = 0;  // this lane's slots per code: code c in byte c & 7 of h[c >> 3]
#pragma unroll
                    for (int k = 0; k < NPT; ++k) {
                        if (id[k] != kNoIdx) {
                            RowX x;
                            x.sd = enf ? s_dom[k * kExactBlock] : -1;
#pragma unroll
                            for (int r = 0; r < kExtMax; ++r)
                                x.ext[r] = (eword >> r & 1) ? ext[r * kExtCol + k * kExactBlock] : 0;
                            x.ad = -1; x.nm = 0; x.na = 0;
                            if (aword != 0) {
                                x.nm = af_mem[k * kExactBlock]; x.na = af_anti[k * kExactBlock];
                                x.ad = af_dom[k * kExactBlock];
                            }
                            const int c = dry_reason<LAB>(u, a0[k], a1[k], a2[k], lab[k], x, sp->cnt,
                                                          reinterpret_cast<const uint64_t *>(zone));
                            const uint64_t one = 1ull << ((c & 7) * 8);
                            h0 += c < 8 ? one : 0ull;
                            h1 += c < 8 ? 0ull : one;
                            if (bytes) A.why_reason[row * A.n + id[k]] = (uint8_t)c;  // consecutive lanes, consecutive bytes
                        }
                        // one slot at a time: eight slots' gathers in flight at once would take their registers from
                        // the rows, which the scan of every pod wants resident
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    // the wave's sums: even and odd bytes widened apart into four 16-bit fields a word (at most 64 lanes
                    // x 8 slots in a field), as ksched_dryrun.hip's hist_flush does; lane c then holds code c's count --
                    // field (c & 7) >> 1 of word (c >> 3) * 2 + (c & 1) -- and adds it to the row where it is not zero
                    constexpr uint64_t kEven = 0x00ff00ff00ff00ffull;
                    const uint64_t s0 = (uint64_t)wave_sum_i64((int64_t)(h0 & kEven));
                    const uint64_t s1 = (uint64_t)wave_sum_i64((int64_t)((h0 >> 8) & kEven));
                    const uint64_t s2 = (uint64_t)wave_sum_i64((int64_t)(h1 & kEven));
                    const uint64_t s3 = (uint64_t)wave_sum_i64((int64_t)((h1 >> 8) & kEven));
                    const uint64_t sw = (lane & 8) ? ((lane & 1) ? s3 : s2) : ((lane & 1) ? s1 : s0);
                    const unsigned long long mine = (sw >> (16 * ((lane & 7) >> 1))) & 0xffffull;
                    if (lane < kNumWhyReasons && mine != 0) atomicAdd(A.why_counts + row * kNumWhyReasons + lane, mine);
                    if (g == 0 && tid == 0) A.why_pod[row] = (int32_t)i;
                }
            }
        } else if (gi == kNoIdx) {
            oidx = -2;  // NO_POSITIVE_SCORE (reference: nil node, anchor/priorities.go:55-62)
        } else {
            oidx = gi;
            osc = PRIO == kPrioPrice ? 0.0 - gk : gk;
#pragma unroll
            for (int k = 0; k < NPT; ++k) {
                if (id[k] == gi) {  // commit: used += request, ONE pod (anchor/predicate.go:99-102)
                    a0[k] = wsub(a0[k], rc); a1[k] = wsub(a1[k], rm); a2[k] = wsub(a2[k], 1);
                    f0[k] = (double)a0[k]; f1[k] = (double)a1[k]; f2[k] = (double)a2[k];
                    y0[k] = recip_or_zero(a0[k], f0[k]); y1[k] = recip_or_zero(a1[k], f1[k]);
                    y2[k] = recip_or_zero(a2[k], f2[k]);
                    if constexpr (EXT) {
                        if (eword != 0) {  // the owner lane: its own slot's words, the non-zero columns only
#pragma unroll
                            for (int r = 0; r < kExtMax; ++r)
                                if (eword >> r & 1) {
                                    int64_t *w = ext + r * kExtCol + k * kExactBlock;
                                    *w = wsub(*w, er[r]);
                                }
                        }
                    }
                    if constexpr (AFF) {
                        if (aword != 0) {  // the owner lane: its own slot's words; node_anti_zone is read by no test
                            if constexpr (FULL) {
                                if (logit) {  // the words before the OR, for this lane's own walk of a rejected gang
                                    uint64_t *u = A.af_undo_slot + gs.gm * 3;
                                    u[0] = af_mem[k * kExactBlock];
                                    u[1] = af_anti[k * kExactBlock];
                                    if (paz != 0) u[2] = A.af_anti_zone[gi];
                                }
                            }
                            af_mem[k * kExactBlock] |= pmem;
                            af_anti[k * kExactBlock] |= pah;
                            if (paz != 0) A.af_anti_zone[gi] |= paz;
                        }
                    }
                }
            }
        }
        if (g == 0 && tid == 0) {
            A.out.idx[i] = oidx;
            A.out.score[i] = osc;
            A.out.feas[i] = (int32_t)gc;
        }
        if constexpr (AFF) {
            if (aword != 0 && oidx >= 0) {  // (the same in every thread of every workgroup)
                any_host |= pmem;
                // uniform inputs only -- the pod's words and the winner's domain, a load from an array nobody writes --
                // decide the barrier: never the zone words themselves, which thread 0 is about to overwrite
                if ((pmem | paz) != 0) {
                    const int32_t wd = A.af_dom[__builtin_amdgcn_readfirstlane(oidx)];
                    if (wd >= 0) {
                        any_zone |= pmem;
                        if (tid == 0) {
                            if constexpr (FULL) {
                                if (logit) {  // this workgroup's copy before the OR, for thread 0's own walk
                                    uint64_t *u = A.af_undo_zone + ((size_t)g * kGangMax + gs.gm) * 2;
                                    u[0] = zone[wd].member;
                                    u[1] = zone[wd].anti;
                                }
                            }
                            zone[wd].member |= pmem; zone[wd].anti |= paz;
                        }
                        __syncthreads();  // the next pod's gathers come before its first barrier
                    }
                }
            }
        }
        if constexpr (SPREAD) {
            if (sword >= 0 && oidx >= 0) {  // (the same in every thread of every workgroup)
                const int32_t wd = A.sp_dom[__builtin_amdgcn_readfirstlane(oidx)];
                if (wd >= 0) {
                    if (tid == 0) {
                        const int32_t s = sword >> 1;
                        int32_t *row = sp->cnt + s * A.sp_D;
                        const int32_t old = row[wd];
                        row[wd] = old + 1;
                        if (old == sp->mn[s] && --sp->nmin[s] == 0) {
                            // the row's last domain at the minimum: every domain now holds at least old + 1
                            int32_t nm = 0;
                            for (int d = 0; d < A.sp_D; ++d) nm += row[d] == old + 1;
                            sp->mn[s] = old + 1; sp->nmin[s] = nm;
                        }
                    }
                    __syncthreads();  // the next pod's gathers come before its first barrier
                }
            }
        }
        if constexpr (GANG) {
            if (tid == 0) s_log[gs.gm] = oidx;
            gs.placed += oidx >= 0;
            ++gs.gm;
            if (gend != 0) {  // the gang's last member: accept or roll back (the same answer in every workgroup)
                const int32_t gsize = gend & 0xffff;
                const bool reject = gs.placed < (gend >> 16);
                if (reject && gs.placed > 0) {
                    __syncthreads();  // the log's last entry
                    const int64_t first = i + 1 - gsize;
                    uint32_t dirty = 0;
                    [[maybe_unused]] bool moved = false;  // ALL: the walk decremented a count of the spread table
#pragma nounroll
                    for (int32_t mm = 0; mm < gsize; ++mm) {
                        // FULL: newest first -- a word logged several times ends at its oldest value (the other undos
                        // are sums: any order)
                        const int32_t m = FULL ? gsize - 1 - mm : mm;
                        const int32_t li = s_log[m];
                        if (li < 0) continue;  // a member that failed keeps its own code
                        if (g == 0 && tid == 0) { A.out.idx[first + m] = kGangRejected; A.out.score[first + m] = 0.0; }
                        const int64_t urc = A.pods.rc[first + m], urm = A.pods.rm[first + m];
                        [[maybe_unused]] const int32_t uew = ALL ? A.ext_word[first + m] : 0;
                        // FULL: the member's affinity word and, where set, its member and anti_zone words (uniform); a
                        // rejected gang of placed members is never a gang of one, so every such member was logged
                        [[maybe_unused]] const int32_t uaw = FULL ? A.af_word[first + m] : 0;
                        [[maybe_unused]] uint64_t upm = 0, upz = 0;
                        if constexpr (FULL) {
                            if (uaw != 0) {
                                upm = A.af_pod[(first + m) * kAffWords];
                                upz = A.af_pod[(first + m) * kAffWords + 2];
                            }
                        }
#pragma unroll
                        for (int k = 0; k < NPT; ++k) {
                            if (id[k] == li) {  // the commit's inverse: a wrapping add undoes the wrapping subtract
                                a0[k] = wadd(a0[k], urc); a1[k] = wadd(a1[k], urm); a2[k] = wadd(a2[k], 1);
                                dirty |= 1u << k;
                                if constexpr (FULL) {
                                    if (uaw != 0) {  // the owner lane: what it logged itself at this member's commit
                                        const uint64_t *u = A.af_undo_slot + m * 3;
                                        af_mem[k * kExactBlock] = u[0];
                                        af_anti[k * kExactBlock] = u[1];
                                        if (upz != 0) A.af_anti_zone[li] = u[2];
                                    }
                                }
                                if constexpr (ALL) {
                                    if (uew != 0) {  // the owner lane: the member's non-zero requests back to its own words
#pragma unroll
                                        for (int r = 0; r < kExtMax; ++r)
                                            if (uew >> r & 1) {
                                                int64_t *w = ext + r * kExtCol + k * kExactBlock;
                                                *w = wadd(*w, A.ext_req[(first + m) * kExtMax + r]);
                                            }
                                    }
                                }
                            }
                        }
                        if constexpr (ALL) {
                            const int32_t usw = A.sp_word[first + m];
                            if (usw >= 0) {  // (the same in every thread of every workgroup, as the increment was)
                                const int32_t wd = A.sp_dom[__builtin_amdgcn_readfirstlane(li)];
                                if (wd >= 0) {
                                    moved = true;
                                    if (tid == 0) {
                                        // the row's minimum and its holders stay what a fresh load would count: a value
                                        // below the minimum is the new minimum, held once; one equal to it, one more holder
                                        const int32_t s = usw >> 1;
                                        int32_t *row = sp->cnt + s * A.sp_D;
                                        const int32_t v = row[wd] - 1;
                                        row[wd] = v;
                                        if (v < sp->mn[s]) { sp->mn[s] = v; sp->nmin[s] = 1; }
                                        else if (v == sp->mn[s]) ++sp->nmin[s];
                                    }
                                }
                            }
                        }
                        if constexpr (FULL) {
                            if (uaw != 0 && (upm | upz) != 0) {  // (the same in every thread, as the commit's condition was)
                                const int32_t wd = A.af_dom[__builtin_amdgcn_readfirstlane(li)];
                                if (wd >= 0) {
                                    moved = true;
                                    if (tid == 0) {  // what thread 0 logged itself at this member's commit
                                        const uint64_t *u = A.af_undo_zone + ((size_t)g * kGangMax + m) * 2;
                                        zone[wd].member = u[0];
                                        zone[wd].anti = u[1];
                                    }
                                }
                            }
                        }
                    }
                    if constexpr (FULL) { any_host = sv_host; any_zone = sv_zone; }
                    if constexpr (ALL) {
                        if (moved) __syncthreads();  // the next pod's gathers come before its first barrier
                    }
#pragma unroll
                    for (int k = 0; k < NPT; ++k) {
                        if (dirty >> k & 1) {
                            f0[k] = (double)a0[k]; f1[k] = (double)a1[k]; f2[k] = (double)a2[k];
                            y0[k] = recip_or_zero(a0[k], f0[k]); y1[k] = recip_or_zero(a1[k], f1[k]);
                            y2[k] = recip_or_zero(a2[k], f2[k]);
                        }
                    }
                }
                if (g == 0 && tid == 0 && A.gang_placed) A.gang_placed[gs.gang] = reject ? 0 : gs.placed;
                ++gs.gang; gs.gm = 0; gs.placed = 0;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NPT; ++k)
        if (id[k] != kNoIdx) set_node(A.nodes + id[k], a0[k], a1[k], a2[k]);
    if constexpr (EXT) {
        for (int r = 0; r < A.n_ext; ++r) {
#pragma unroll
            for (int k = 0; k < NPT; ++k)
                if (id[k] != kNoIdx) A.ext[(int64_t)r * A.n + id[k]] = ext[r * kExtCol + k * kExactBlock];
        }
    }
    if constexpr (AFF) {
        if (af_on) {
#pragma unroll
            for (int k = 0; k < NPT; ++k)
                if (id[k] != kNoIdx) {
                    A.af_member[id[k]] = af_mem[k * kExactBlock];
                    A.af_anti_host[id[k]] = af_anti[k * kExactBlock];
                }
            // (every pod -- and every walk -- that moved the zone table ended with a barrier: the copy is complete in
            // every thread's view)
            if (g == 0) {
                for (int d = tid; d < A.af_D; d += kExactBlock) {
                    A.af_zone[2 * d] = zone[d].member;
                    A.af_zone[2 * d + 1] = zone[d].anti;
                }
                if (tid == 0) { A.af_any[0] = any_host; A.af_any[1] = any_zone; }
            }
        }
    }
    if constexpr (SPREAD) {
        // (every pod that moved the table ended with a barrier: the copy is complete in every thread's view)
        if (g == 0) {
            const int cells = A.sp_S * A.sp_D;
            for (int c = tid; c < cells; c += kExactBlock) A.sp_counts[c] = sp->cnt[c];
        }
    }
    if constexpr (WHY) {
        if (g == 0 && tid == 0) *A.why_nofit = nofit;
    }
}

#if KSCHED_EXACT_PART == 0
// ------------------------------------------------------------------------------------------------
// Exact mode on ONE workgroup (kExact1Block threads; n <= kExact1Block * NPT): every node lives in a register
// slot of this workgroup, so a pod is decided with one workgroup barrier and no cross-workgroup exchange (k_exact
// with G > 1 pays a round of tagged granules through L2 per pod, ~2.7 us on c2).  Thread t holds slots
// s = t + k * kExact1Block.
//   best-price: slot s is the node of rank s in (price asc, node index asc) -- the order of the reference's
//     argmax over -price with the lowest index on ties (README.md:37-64; price_key) -- so a pod's node is the
//     FIRST feasible slot: per wave one ballot per k (its lowest set bit), the minimum over the waves; the feasible
//     count is the sum of the ballots' popcounts.  No key is compared at all.
//   resource: slot s is node s; per pod every lane keys its slots, wave arg-best, the waves' bests through LDS.
// Restated by the same oracle as k_exact (oracle/cpu_ref.c or_schedule); results bit-identical.
// ------------------------------------------------------------------------------------------------
template <int NPT, int BS, int PRIO, int DOM, bool LAB, bool F53>
__global__ __launch_bounds__(BS) void k_exact1(ExactArgs A) {
    constexpr int kExact1Block = BS;
    constexpr int W = kExact1Block / 64;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const double y3 = recip(3.0);
    constexpr bool kRes = PRIO != kPrioPrice;
    int64_t a0[NPT], a1[NPT], a2[NPT];
    double f0[kRes ? NPT : 1], f1[kRes ? NPT : 1], f2[kRes ? NPT : 1];
    double yy0[kRes ? NPT : 1], yy1[kRes ? NPT : 1], yy2[kRes ? NPT : 1];
    uint64_t lab[NPT];
    float pr[NPT];
    int32_t id[NPT];
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const int64_t sl = tid + (int64_t)k * kExact1Block;
        id[k] = kNoIdx;
        a0[k] = a1[k] = a2[k] = 0; lab[k] = 0; pr[k] = 0.f;
        if constexpr (kRes) { f0[k] = f1[k] = f2[k] = 0.0; yy0[k] = yy1[k] = yy2[k] = 0.0; }
        if (sl < A.n) {
            const int32_t j = A.perm ? A.perm[sl] : (int32_t)sl;
            const NodeRec &nd = A.nodes[j];
            a0[k] = nd.a[0]; a1[k] = nd.a[1]; a2[k] = nd.a[2];
            lab[k] = nd.labels; pr[k] = nd.price; id[k] = j;
            if constexpr (kRes) {
                f0[k] = nd.af[0]; f1[k] = nd.af[1]; f2[k] = nd.af[2];
                yy0[k] = nd.y[0]; yy1[k] = nd.y[1]; yy2[k] = nd.y[2];
            }
        }
    }
    __shared__ int32_t s_cnt[2][W];
    __shared__ int32_t s_slot[2][W];  // best-price: the wave's first feasible slot (INT32_MAX: none)
    __shared__ double s_key[2][W];    // resource: the wave's best (key, node)
    __shared__ int32_t s_idx[2][W];
    // the next pod's request is loaded one pod ahead: its latency hides behind the current pod
    int64_t nrc = 0, nrm = 0, nrp = 0;
    uint64_t nsel = 0;
    if (A.pods.p > 0) { nrc = A.pods.rc[0]; nrm = A.pods.rm[0]; nrp = A.pods.rp[0]; nsel = LAB ? A.pods.sel[0] : 0; }
    for (int64_t i = 0; i < A.pods.p; ++i) {
        const int par = (int)(i & 1);
        const int64_t rc = nrc, rm = nrm, rp = nrp;
        const uint64_t sel = nsel;
        if (i + 1 < A.pods.p) {
            nrc = A.pods.rc[i + 1]; nrm = A.pods.rm[i + 1]; nrp = A.pods.rp[i + 1];
            nsel = LAB ? A.pods.sel[i + 1] : 0;
        }
        int32_t cnt = 0;
        int32_t oidx = -1;
        double osc = 0.0;
        if constexpr (!kRes) {
            int32_t first = 0x7fffffff;
#pragma unroll
            for (int k = 0; k < NPT; ++k) {
                const bool f = id[k] != kNoIdx && fits(rc, rm, rp, sel, a0[k], a1[k], a2[k], lab[k], LAB);
                const uint64_t m = __ballot(f);
                cnt += __popcll(m);
                if (first == 0x7fffffff && m) first = k * kExact1Block + wave * 64 + (int)__builtin_ctzll(m);
            }
            if (lane == 0) { s_slot[par][wave] = first; s_cnt[par][wave] = cnt; }
            __syncthreads();
            int32_t gs = s_slot[par][0], gc = s_cnt[par][0];
#pragma unroll
            for (int w = 1; w < W; ++w) { gs = s_slot[par][w] < gs ? s_slot[par][w] : gs; gc += s_cnt[par][w]; }
            // the first feasible slot's owner commits it and writes the pod's results; no feasible node: thread 0
            if (gc == 0) {
                if (tid == 0) { A.out.idx[i] = -1; A.out.score[i] = 0.0; A.out.feas[i] = 0; }  // NO_FIT
            } else if ((gs & (kExact1Block - 1)) == tid) {
#pragma unroll
                for (int k = 0; k < NPT; ++k) {
                    if (gs == k * kExact1Block + tid) {  // commit: used += request, ONE pod (anchor/predicate.go:99-102)
                        A.out.idx[i] = id[k];
                        A.out.score[i] = 0.0 - price_key(pr[k]);
                        A.out.feas[i] = gc;
                        a0[k] = wsub(a0[k], rc); a1[k] = wsub(a1[k], rm); a2[k] = wsub(a2[k], 1);
                    }
                }
            }
            (void)oidx; (void)osc;
        } else {
            const double rcf = (double)rc, rmf = (double)rm, rpf = (double)rp;
            double bk = -__builtin_inf();
            int32_t bi = kNoIdx;
#pragma unroll
            for (int k = 0; k < NPT; ++k) {
                if (id[k] != kNoIdx) {
                    const bool f = fits(rc, rm, rp, sel, a0[k], a1[k], a2[k], lab[k], LAB);
                    cnt += f;
                    double key;
                    if (pair_key_fast<PRIO, DOM, F53>(f, rc, rm, rp, rcf, rmf, rpf, a0[k], a1[k], a2[k], f0[k], f1[k],
                                                      f2[k], yy0[k], yy1[k], yy2[k], y3, pr[k], &key) &&
                        better(key, id[k], bk, bi)) {
                        bk = key;
                        bi = id[k];
                    }
                }
            }
            int32_t aux = 0;
            wave_argbest(bk, bi, aux);
            cnt = (int32_t)wave_sum_i64(cnt);
            if (lane == 0) { s_key[par][wave] = bk; s_idx[par][wave] = bi; s_cnt[par][wave] = cnt; }
            __syncthreads();
            double gk = s_key[par][0];
            int32_t gi = s_idx[par][0], gc = s_cnt[par][0];
#pragma unroll
            for (int w = 1; w < W; ++w) {
                gc += s_cnt[par][w];
                if (better(s_key[par][w], s_idx[par][w], gk, gi)) { gk = s_key[par][w]; gi = s_idx[par][w]; }
            }
            oidx = gc == 0 ? -1 : (gi == kNoIdx ? -2 : gi);  // NO_FIT / NO_POSITIVE_SCORE (anchor/schedule.go:74-76)
            osc = oidx >= 0 ? gk : 0.0;
            if (oidx >= 0) {
#pragma unroll
                for (int k = 0; k < NPT; ++k) {
                    if (id[k] == gi) {
                        a0[k] = wsub(a0[k], rc); a1[k] = wsub(a1[k], rm); a2[k] = wsub(a2[k], 1);
                        f0[k] = (double)a0[k]; f1[k] = (double)a1[k]; f2[k] = (double)a2[k];
                        yy0[k] = recip_or_zero(a0[k], f0[k]); yy1[k] = recip_or_zero(a1[k], f1[k]);
                        yy2[k] = recip_or_zero(a2[k], f2[k]);
                    }
                }
            }
            if (tid == 0) { A.out.idx[i] = oidx; A.out.score[i] = osc; A.out.feas[i] = gc; }
        }
    }
#pragma unroll
    for (int k = 0; k < NPT; ++k)
        if (id[k] != kNoIdx) set_node(A.nodes + id[k], a0[k], a1[k], a2[k]);
}

#endif  // KSCHED_EXACT_PART == 0

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
namespace {

// kRunFull, kRunFullWhy (parts 2, 3): hipFuncAttributeMaxDynamicSharedMemorySize belongs to a kernel on ONE device, and a context chooses
// its device: the (device ordinal, kernel) pairs that have it, set at the pair's first launch as launch_stream_kernel
// does.  Contexts run on threads of their own.
[[maybe_unused]] hipError_t full_lds_limit(const void *fn, size_t most) {
    static std::mutex mu;
    static std::set<std::pair<int, const void *>> have;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(mu);
    if (have.count({dev, fn})) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
    if (e == hipSuccess) have.insert({dev, fn});
    return e;
}

template <int NPT, int PRIO, int DOM, bool LAB, bool F53, ExactRun RUN>
hipError_t exact_one(const ExactArgs &a, int block, bool coop, hipStream_t s) {
    constexpr ExactKind K = exact_kind(RUN);
    auto fn = k_exact<NPT, PRIO, DOM, LAB, F53, RUN>;
    // ext: the workgroup's slots of every column (ext_table), at most kExtMax * 256 * 8 * 8 B = 64 KiB (no table:
    // n_ext == 0, none)
    // aff: the workgroup's slots of node_member and node_anti_host and their domains (aff_table), at most 256 * 8 * 20 B
    // = 40 KiB beside the 16 KiB static zone table, and only where the call has a table
    // both: the affinity words behind the columns, up to 104 KiB, beyond the 64 KiB a kernel is admitted to by default
    // -- so the kernel's first launch on a device raises its limit to the kind's maximum there (full_lds_limit)
    constexpr size_t aff = (size_t)kExactBlock * NPT * (2 * sizeof(uint64_t) + sizeof(int32_t));
    const size_t cols = K.ext ? (size_t)a.n_ext * kExactBlock * NPT * sizeof(int64_t) : 0;
    const size_t lds = cols + (K.aff && a.af_dom ? aff : 0);
    if ((K.ext || K.aff) && block != kExactBlock) return hipErrorInvalidValue;
    if constexpr (K.ext && K.aff) {
        if (a.n_ext < 0 || a.n_ext > kExtMax) return hipErrorInvalidValue;
        const hipError_t e = full_lds_limit((const void *)fn, (size_t)kExtMax * kExactBlock * NPT * sizeof(int64_t) + aff);
        if (e != hipSuccess) return e;
    }
    if (coop && a.G > 1) {
        ExactArgs copy = a;
        void *args[] = {&copy};
        return hipLaunchCooperativeKernel((const void *)fn, dim3(a.G), dim3(block), args, lds, s);
    }
    hipLaunchKernelGGL(fn, dim3(a.G), dim3(block), lds, s, a);
    return hipGetLastError();
}

template <int PRIO, int DOM, bool LAB, bool F53, ExactRun RUN>
hipError_t exact_npt(int npt, const ExactArgs &a, int block, bool coop, hipStream_t s) {
    switch (npt) {
        case 1: return exact_one<1, PRIO, DOM, LAB, F53, RUN>(a, block, coop, s);
        case 2: return exact_one<2, PRIO, DOM, LAB, F53, RUN>(a, block, coop, s);
        case 4: return exact_one<4, PRIO, DOM, LAB, F53, RUN>(a, block, coop, s);
        case 8: return exact_one<8, PRIO, DOM, LAB, F53, RUN>(a, block, coop, s);
        default: return hipErrorInvalidValue;
    }
}

#if KSCHED_EXACT_PART == 0
template <int PRIO, int DOM, bool LAB, bool F53>
hipError_t exact_run(ExactRun run, int npt, const ExactArgs &a, int block, bool coop, hipStream_t s) {
    switch (run) {
        case kRunPlain: return exact_npt<PRIO, DOM, LAB, F53, kRunPlain>(npt, a, block, coop, s);
        case kRunGang: return exact_npt<PRIO, DOM, LAB, F53, kRunGang>(npt, a, block, coop, s);
        case kRunSpread: return exact_npt<PRIO, DOM, LAB, F53, kRunSpread>(npt, a, block, coop, s);
        case kRunExt: return exact_npt<PRIO, DOM, LAB, F53, kRunExt>(npt, a, block, coop, s);
        case kRunAll: return exact_npt<PRIO, DOM, LAB, F53, kRunAll>(npt, a, block, coop, s);
        case kRunAffinity: break;  // (part 1: launch_exact_affinity)
        case kRunFull: break;      // (part 2: launch_exact_full)
        case kRunFullWhy: break;   // (part 3: launch_exact_full_why)
    }
    return hipErrorInvalidValue;
}

template <int NPT, int BS, int PRIO, int DOM, bool LAB, bool F53>
hipError_t exact1_one(const ExactArgs &a, hipStream_t s) {
    hipLaunchKernelGGL((k_exact1<NPT, BS, PRIO, DOM, LAB, F53>), dim3(1), dim3(BS), 0, s, a);
    return hipGetLastError();
}
// (npt, block): resource slots <= 4 per thread of 1024 (registers); best-price more
template <int PRIO, int DOM, bool LAB, bool F53>
hipError_t exact1_npt(int npt, int bs, const ExactArgs &a, hipStream_t s) {
    if (bs == 1024) {
        switch (npt) {
            case 1: return exact1_one<1, 1024, PRIO, DOM, LAB, F53>(a, s);
            case 2: return exact1_one<2, 1024, PRIO, DOM, LAB, F53>(a, s);
            case 3: return exact1_one<3, 1024, PRIO, DOM, LAB, F53>(a, s);
            case 4: return exact1_one<4, 1024, PRIO, DOM, LAB, F53>(a, s);
            default: break;
        }
        if constexpr (PRIO == kPrioPrice) {
            switch (npt) {
                case 5: return exact1_one<5, 1024, PRIO, DOM, LAB, F53>(a, s);
                case 6: return exact1_one<6, 1024, PRIO, DOM, LAB, F53>(a, s);
                case 8: return exact1_one<8, 1024, PRIO, DOM, LAB, F53>(a, s);
                case 12: return exact1_one<12, 1024, PRIO, DOM, LAB, F53>(a, s);
                case 16: return exact1_one<16, 1024, PRIO, DOM, LAB, F53>(a, s);
                default: return hipErrorInvalidValue;
            }
        }
        return hipErrorInvalidValue;
    }
    if constexpr (PRIO == kPrioPrice) {
        if (bs == 512 && npt == 10) return exact1_one<10, 512, PRIO, DOM, LAB, F53>(a, s);
        if (bs == 256 && npt == 20) return exact1_one<20, 256, PRIO, DOM, LAB, F53>(a, s);
    }
    return hipErrorInvalidValue;
}
#endif  // KSCHED_EXACT_PART == 0

}  // namespace

#if KSCHED_EXACT_PART == 0
hipError_t launch_exact(ExactRun run, int npt, int prio, int dom, bool lab, bool f53, const ExactArgs &a, int block,
                        bool coop, hipStream_t s) {
    if (run < kRunPlain || run > kRunFullWhy) return hipErrorInvalidValue;
    // the fields of ExactArgs, constraint by constraint: the per-pod words always, the table's "off" form (sp_S == 0,
    // n_ext == 0, af_dom null) accepted only where the kind is optional
    const ExactKind k = exact_kind(run);
    const bool spread_ok = a.sp_word && ((k.optional && a.sp_S == 0) ||
                                         (a.sp_dom && a.sp_counts && a.sp_skew && a.sp_D >= 1 && a.sp_S >= 1 &&
                                          (int64_t)a.sp_D * a.sp_S <= kSpreadMaxCells && a.sp_S <= kSpreadMaxGroups));
    const bool ext_ok = a.ext_word && ((k.optional && a.n_ext == 0) || (a.ext && a.ext_req && a.n_ext >= 1 && a.n_ext <= kExtMax));
    const bool aff_ok = a.af_word && (k.optional && !a.af_dom
                                          ? a.af_D == 0
                                          : a.af_dom && a.af_member && a.af_anti_host && a.af_anti_zone && a.af_zone &&
                                                a.af_any && a.af_pod && a.af_D >= 0 && a.af_D <= kSpreadMaxDomains);
    // (the reasons: rows of bytes only where there are rows at all)
    const bool why_ok = a.why_nofit && a.why_rows >= 0 && a.why_node_rows >= 0 && a.why_node_rows <= a.why_rows &&
                        (a.why_rows == 0 || (a.why_pod && a.why_counts)) && (a.why_node_rows == 0 || a.why_reason);
    if ((k.gang && !a.gang_end) || (k.spread && !spread_ok) || (k.ext && !ext_ok) || (k.aff && !aff_ok) ||
        (k.undo && (!a.af_undo_slot || !a.af_undo_zone)) || (k.why && !why_ok))
        return hipErrorInvalidValue;
    if (run == kRunAffinity) return launch_exact_affinity(npt, prio, dom, lab, f53, a, block, coop, s);
    if (run == kRunFull) return launch_exact_full(npt, prio, dom, lab, f53, a, block, coop, s);
    if (run == kRunFullWhy) return launch_exact_full_why(npt, prio, dom, lab, f53, a, block, coop, s);
    KSCHED_DISPATCH(prio, dom, lab, f53, (exact_run<P_, D_, L_, F_>(run, npt, a, block, coop, s)));
}

hipError_t launch_exact1(int npt, int bs, int prio, int dom, bool lab, bool f53, const ExactArgs &a, hipStream_t s) {
    KSCHED_DISPATCH(prio, dom, lab, f53, (exact1_npt<P_, D_, L_, F_>(npt, bs, a, s)));
}
#elif KSCHED_EXACT_PART == 1
hipError_t launch_exact_affinity(int npt, int prio, int dom, bool lab, bool f53, const ExactArgs &a, int block, bool coop,
                                 hipStream_t s) {
    KSCHED_DISPATCH(prio, dom, lab, f53, (exact_npt<P_, D_, L_, F_, kRunAffinity>(npt, a, block, coop, s)));
}
#elif KSCHED_EXACT_PART == 2
hipError_t launch_exact_full(int npt, int prio, int dom, bool lab, bool f53, const ExactArgs &a, int block, bool coop,
                             hipStream_t s) {
    KSCHED_DISPATCH(prio, dom, lab, f53, (exact_npt<P_, D_, L_, F_, kRunFull>(npt, a, block, coop, s)));
}
#else
hipError_t launch_exact_full_why(int npt, int prio, int dom, bool lab, bool f53, const ExactArgs &a, int block, bool coop,
                                 hipStream_t s) {
    KSCHED_DISPATCH(prio, dom, lab, f53, (exact_npt<P_, D_, L_, F_, kRunFullWhy>(npt, a, block, coop, s)));
}
#endif

}  // namespace ksched

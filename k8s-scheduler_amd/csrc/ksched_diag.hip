// ksched_diag.hip -- libksched: diagnostics.  The one reader of the environment, the trace and stamp printers, the
// dump writers, and the decoding of the device error word.  Nothing here is on a call's hot path.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ksched_ctx.h"

namespace ksched {

static int env_int(const char *name, int dflt) {
    const char *v = std::getenv(name);
    return v && *v ? std::atoi(v) : dflt;
}
static std::string env_str(const char *name) {
    const char *v = std::getenv(name);
    return v ? v : "";
}

void read_env(ksched_diag *d) {
    d->trace = env_int("KSCHED_PERSIST_TRACE", 0) != 0;
    d->trace_dump = env_str("KSCHED_TRACE_DUMP");
    d->trace_wg = env_str("KSCHED_TRACE_WG");
    d->xchg_dump = env_str("KSCHED_XCHG_DUMP");
    d->commit_stamps = env_int("KSCHED_COMMIT_STAMPS", 0) != 0;
    d->merge_stamps = env_int("KSCHED_MERGE_STAMPS", 0) != 0;
    d->debug = env_int("KSCHED_DEBUG", 0) != 0;
    d->no_screen = env_int("KSCHED_NO_SCREEN", 0) != 0;
    d->no_pairs = env_int("KSCHED_NO_PAIRS", 0) != 0;
    d->no_seed = env_int("KSCHED_NO_SEED", 0) != 0;
    d->touch_screen = env_int("KSCHED_NO_TOUCH_SCREEN", 0) == 0;
    d->no_fold_mask = env_int("KSCHED_NO_FOLD_MASK", 0) != 0;
    d->early_inh = env_int("KSCHED_NO_EARLY_INH", 0) == 0;
    d->poison = env_int("KSCHED_POISON", 0) != 0;
    if (const std::string f = env_str("KSCHED_LDS_FILL"); !f.empty()) d->lds_fill = (uint32_t)std::strtoul(f.c_str(), nullptr, 0);
    d->lds_role = env_int("KSCHED_LDS_ROLE", 7);
    d->lds_lo = env_int("KSCHED_LDS_LO", 0);
    if (!env_str("KSCHED_LDS_HI").empty()) d->lds_hi = env_int("KSCHED_LDS_HI", 0);
    d->jitter = (uint32_t)env_int("KSCHED_JITTER", 0);
    d->plain_launch = env_int("KSCHED_PLAIN_LAUNCH", 0) != 0;
    d->exact1_bs = env_int("KSCHED_EXACT1_BS", 1024);
    d->xchg_diag = env_int("KSCHED_XCHG_DIAG", 0);
    d->epoch_base = env_int("KSCHED_XCHG_EPOCH_BASE", 0);
    d->persist_timeout_ms = env_int("KSCHED_PERSIST_TIMEOUT_MS", 10000);
    d->exchange_timeout_ms = env_int("KSCHED_EXCHANGE_TIMEOUT_MS", 2000);
    d->rescue_max = env_int("KSCHED_RESCUE_MAX", 4);
    d->rescue_rate = env_int("KSCHED_RESCUE_RATE", 4);
    d->rescue_cap = env_int("KSCHED_RESCUE_CAP", 16);
    d->rescue_low = env_int("KSCHED_RESCUE_LOW", 2);
    d->rescue_look = env_int("KSCHED_RESCUE_LOOK", 0);
}

static void write_u64(const std::string &path, const int64_t *hdr, size_t nhdr, const std::vector<uint64_t> &t) {
    if (FILE *f = std::fopen(path.c_str(), "wb")) {
        if (nhdr) std::fwrite(hdr, 8, nhdr, f);
        std::fwrite(t.data(), 8, t.size(), f);
        std::fclose(f);
    }
}

// KSCHED_PERSIST_TRACE=1: mean per-batch phase times of the last persistent run, to stderr (us)
void print_persist_trace(ksched_ctx *c) {
    std::vector<uint64_t> t((size_t)c->trace_rows() * kTraceCols);
    if (hipMemcpy(t.data(), c->d->trace, t.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    // KSCHED_TRACE_DUMP=<path>: the raw stamps for offline percentiles
    if (!c->diag.trace_dump.empty()) write_u64(c->diag.trace_dump, nullptr, 0, t);
    auto at = [&](int64_t b, int col) { return t[(size_t)b * kTraceCols + col]; };
    double sum[16] = {};
    // WG 0 wave 0, screened batches: pass 1 (seeded scan: the seed pass), bound merge, pass 2 (seeded scan: the single
    // pass), exact phase (sums), exact rows, and the wait for the other waves' pass 1 (stamp 37, behind the barrier)
    double scr[6] = {};
    int64_t nscr = 0, npair = 0;
    double pairs_sum = 0;  // WG 0: batches whose exact phase ran over the pair lists, and their pairs
    int64_t cnt = 0, first = -1, last = -1;
    constexpr int64_t L = kPipeLag;
    for (int64_t b = L; b < c->trace_rows(); ++b) {
        if (!at(b, 0) || !at(b, 1) || !at(b, 2) || !at(b, 3) || !at(b, 4) || !at(b - L, 4)) continue;
        if (first < 0) first = b;
        last = b;
        ++cnt;
        sum[0] += (double)(int64_t)(at(b, 0) - at(b - L, 4));  // commit(b-L) end -> score(b) start
        sum[1] += (double)(int64_t)(at(b, 1) - at(b, 0));      // score (WG 0 start -> last arrival)
        sum[2] += (double)(int64_t)(at(b, 2) - at(b, 1));      // merge
        sum[3] += (double)(int64_t)(at(b, 3) - at(b, 2));      // last merge -> commit start
        sum[4] += (double)(int64_t)(at(b, 4) - at(b, 3));      // commit
        sum[5] += (double)(int64_t)(at(b, 3) - at(b - 1, 4));  // commit(b-1) end -> commit(b) start
        sum[6] += (double)(int64_t)(at(b, 6) - at(b - L, 4));  // WG 0: commit(b-L) end -> its poll returns
        sum[7] += (double)(int64_t)(at(b, 0) - at(b, 6));      // WG 0: plan loads + XBuf apply
        sum[8] += (double)(int64_t)(at(b, 5) - at(b, 0));      // WG 0: score + fold + list stores
        sum[9] += (double)(int64_t)(at(b, 7) - at(b, 1));      // last arrival -> merger past its poll
        sum[10] += (double)(int64_t)(at(b, 8) - at(b, 0));     // WG 0 wave 0: row loop (incl. pod loads)
        sum[11] += (double)(int64_t)(at(b, 9) - at(b, 8));     // WG 0: waiting for its slowest wave
        sum[12] += (double)(int64_t)(at(b, 10) - at(b, 9));    // WG 0: fold
        sum[13] += (double)(int64_t)(at(b, 5) - at(b, 10));    // WG 0: list stores + drain
        sum[14] += (double)(int64_t)(at(b, 15) - at(b - 1, 4));  // commit(b-1) end -> commit loop top of b
        sum[15] += (double)(int64_t)(at(b, 3) - at(b, 15));      // commit loop top -> past the merge wait
        if (at(b, 11) && at(b, 12)) {  // a screened batch (ksched_pipe.hip score_role)
            ++nscr;
            scr[0] += (double)(int64_t)(at(b, 11) - at(b, 0));
            const uint64_t bar = at(b, 37) ? at(b, 37) : at(b, 11);
            scr[5] += (double)(int64_t)(bar - at(b, 11));
            scr[1] += (double)(int64_t)(at(b, 12) - bar);
            scr[2] += (double)(int64_t)(at(b, 14) - at(b, 12));
            scr[3] += (double)(int64_t)(at(b, 8) - at(b, 14));
            scr[4] += (double)(uint32_t)at(b, 13);
            const uint32_t pairs = (uint32_t)(at(b, 13) >> 32);
            if (pairs != 0xffffffffu) { ++npair; pairs_sum += pairs; }
        }
    }
    if (c->d->dbg) {
        int64_t hd[kCommitDbgWords];
        if (hipMemcpy(hd, c->d->dbg, sizeof(hd), hipMemcpyDeviceToHost) == hipSuccess && hd[14] && hd[16])
            fprintf(stderr, "persist commit screen: export(b-1) entries %lld keyed exactly %.4f | guessed columns %lld, "
                    "exactly %.4f | sequential columns %lld, exactly %.4f | rescue re-keys %lld\n", (long long)hd[16],
                    (double)hd[17] / std::max<int64_t>(1, hd[16]), (long long)hd[18], (double)hd[19] / std::max<int64_t>(1, hd[18]),
                    (long long)hd[20], (double)hd[21] / std::max<int64_t>(1, hd[20]), (long long)hd[22]);
        if (hd[14])
            fprintf(stderr, "persist commit guess: iterations %lld, of them past the two lowest entries (all K scanned) %lld | "
                    "pods resolved one by one %lld\n", (long long)hd[5], (long long)hd[8], (long long)hd[31]);
        if (hd[14])
            fprintf(stderr, "persist commit: batches=%lld rounds/batch %.3f guess iterations/round %.2f failures %lld | "
                    "cycles/batch: before the wait %.0f (other waves %.0f) entry to past the wait %.0f (poll %.0f, poll + barrier %.0f, early read sufficed %.3f, early inh read sufficed %lld of %lld) | prologue %.0f guess %.0f evaluate %.0f check %.0f total %.0f\n",
                    (long long)hd[14], (double)hd[12] / hd[14], (double)hd[5] / std::max<int64_t>(1, hd[12]),
                    (long long)hd[13], (double)hd[6] / hd[14], (double)hd[9] / hd[14] / 11.0, (double)hd[7] / hd[14], (double)hd[10] / hd[14], (double)hd[11] / hd[14], (double)hd[15] / hd[14], (long long)hd[29], (long long)hd[30], (double)hd[0] / hd[14],
                    (double)hd[1] / hd[14], (double)hd[2] / hd[14], (double)hd[3] / hd[14], (double)hd[4] / hd[14]);
        if (hd[14])  // a step whose commit made some lane's best touched slot worse rescanned before the rb2 bound
            fprintf(stderr, "persist commit rescans: steps with a worsened holder %lld, every holder kept %lld | plain rescans "
                    "%lld, %.0f cycles each | with the second-best key %lld, %.0f cycles each\n", (long long)hd[23],
                    (long long)hd[24], (long long)hd[25], (double)hd[26] / std::max<int64_t>(1, hd[25]), (long long)hd[27],
                    (double)hd[28] / std::max<int64_t>(1, hd[27]));
        if (hd[14] && hd[16])  // the screened commit's fold masks (KSCHED_NO_FOLD_MASK=1: every wave, every column)
            fprintf(stderr, "persist commit fold masks: checks that read no partials %lld of %lld, partial rows read %lld | "
                    "wave-0 states that read none %lld of %lld | confirm-fold columns visited %lld skipped %lld | batches "
                    "with a check that read none after one that read some %lld\n", (long long)hd[32], (long long)hd[12],
                    (long long)hd[33], (long long)hd[34], (long long)hd[14], (long long)hd[35], (long long)hd[36],
                    (long long)hd[37]);
    }
    if (c->d->mdbg) {
        int64_t hm[8];
        if (hipMemcpy(hm, c->d->mdbg, sizeof(hm), hipMemcpyDeviceToHost) == hipSuccess && hm[7]) {
            const double nwg = (double)hm[7];
            fprintf(stderr, "persist merge: merges=%lld | cycles/merge: loads %.0f rank-heads %.0f barrier %.0f "
                    "global-heads %.0f rank-entries %.0f write %.0f\n", (long long)hm[7], hm[0] / nwg, hm[1] / nwg,
                    hm[2] / nwg, hm[3] / nwg, hm[4] / nwg, hm[5] / nwg);
        }
    }
    if (!cnt) return;
    const double us = 0.01 / (double)cnt;  // 100 MHz ticks -> us, mean
    fprintf(stderr,
            "persist trace: %lld batches, period %.2f us | to-score %.2f score %.2f merge %.2f to-commit %.2f "
            "commit %.2f commit-gap %.2f (to loop top %.2f, top to past the wait %.2f) | wg0: poll %.2f apply %.2f "
            "score %.2f (rows %.2f slowest-wave %.2f fold %.2f stores %.2f) | merger poll %.2f\n",
            (long long)cnt, 0.01 * (double)(int64_t)(at(last, 4) - at(first, 4)) / (double)std::max<int64_t>(1, last - first),
            sum[0] * us, sum[1] * us, sum[2] * us, sum[3] * us, sum[4] * us, sum[5] * us, sum[14] * us, sum[15] * us, sum[6] * us, sum[7] * us,
            sum[8] * us, sum[10] * us, sum[11] * us, sum[12] * us, sum[13] * us, sum[9] * us);
    if (nscr)
        fprintf(stderr, "persist screen (WG 0 wave 0): %lld of %lld batches screened | pass 1 / seed pass %.2f us, other waves "
                "%.2f us, bound %.2f us, pass 2 / single pass %.2f us, exact phase %.2f us (%.2f of the workgroup's %d rows needed; pair lists in %lld batches, "
                "%.1f pairs each)\n", (long long)nscr, (long long)cnt,
                0.01 * scr[0] / nscr, 0.01 * scr[5] / nscr, 0.01 * scr[1] / nscr, 0.01 * scr[2] / nscr, 0.01 * scr[3] / nscr, scr[4] / nscr,
                c->prog_rows, (long long)npair, npair ? pairs_sum / (double)npair : 0.0);
}

// The stream pipeline's KSCHED_MERGE_STAMPS line (after the run's last enqueue; waits for the run).
int print_merge_stamps(ksched_ctx *c) {
    int64_t hm[8];
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(hm, c->d->mdbg, sizeof(hm), hipMemcpyDeviceToHost));
    const double nwg = hm[7] ? (double)hm[7] : 1.0;
    std::fprintf(stderr, "[ksched merge stamps] workgroups=%lld | cycles/wg: loads %.0f rank-heads %.0f barrier %.0f "
                 "global-heads %.0f rank-entries %.0f write %.0f\n", (long long)hm[7], hm[0] / nwg, hm[1] / nwg,
                 hm[2] / nwg, hm[3] / nwg, hm[4] / nwg, hm[5] / nwg);
    return KSCHED_OK;
}

// The stream pipeline's KSCHED_COMMIT_STAMPS line (spc: the speculative commit's; skipped: Ctl::stats[3]).
int print_commit_stamps(ksched_ctx *c, bool spc_commit, int64_t skipped) {
    int64_t hd[16];
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(hd, c->d->dbg, sizeof(hd), hipMemcpyDeviceToHost));
    if (spc_commit)
        std::fprintf(stderr, "[ksched commit_spc] kernels=%lld rounds=%lld failures=%lld (%.3f rounds/batch) | "
                     "cycles/kernel: prologue %.0f guess %.0f evaluate %.0f check %.0f total %.0f\n",
                     (long long)hd[14], (long long)hd[12], (long long)hd[13], (double)hd[12] / (hd[14] ? hd[14] : 1),
                     (double)hd[0] / hd[14], (double)hd[1] / hd[14], (double)hd[2] / hd[14], (double)hd[3] / hd[14],
                     (double)hd[4] / hd[14]);
    else
        std::fprintf(stderr, "[ksched commit stamps] pods=%lld kernels=%lld touched=%lld | cycles/pod: loads+rescore %.0f "
                     "reduce %.0f decide %.0f commit+store %.0f | loop cycles/pod %.0f | skipped %lld\n",
                     (long long)hd[5], (long long)hd[7], (long long)hd[6], (double)hd[0] / hd[5], (double)hd[1] / hd[5],
                     (double)hd[2] / hd[5], (double)hd[3] / hd[5], (double)hd[4] / hd[5], (long long)skipped);
    return KSCHED_OK;
}

// KSCHED_XCHG_DUMP=<path>: the exchange's message hashes, to <path>.r<rank>.c<call> ([cap][B][R + 1] u64)
void dump_xchg(ksched_ctx *c) {
    std::vector<uint64_t> t(c->d->xdbg.bytes / 8);
    if (hipMemcpy(t.data(), c->d->xdbg, t.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    write_u64(c->diag.xchg_dump + ".r" + std::to_string(c->o.rank) + ".c" + std::to_string(c->xdbg_calls), nullptr, 0, t);
}

// KSCHED_TRACE_WG=<path>: the raw per-workgroup stamps ([batches][G] u64: scan start | arrival << 32)
void dump_trace_wg(ksched_ctx *c) {
    std::vector<uint64_t> t((size_t)c->trace_wg_elems());
    if (hipMemcpy(t.data(), c->d->trace_wg, t.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    const int64_t hdr[2] = {(int64_t)c->prog_G, c->trace_wg_elems() / c->prog_G};
    write_u64(c->diag.trace_wg, hdr, 2, t);
}

// KSCHED_PERSIST_TRACE: per score workgroup the summed scan time and poll-end -> arrival time, slowest first,
// with where it ran and whether a merger workgroup shared its CU (PersistArgs::prog words 2, 3).
void print_wg_busy(ksched_ctx *c) {
    if (!c->d_prog) return;
    const int G = c->prog_G, B = c->prog_B, n = G + B + kCommitWGs;
    std::vector<uint64_t> w((size_t)kProgWords * n);
    if (hipMemcpy(w.data(), c->d_prog, w.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    auto where = [&](int i) { return (uint32_t)(w[kProgWords * i + 1] >> 32); };
    std::vector<int> order(G);
    for (int g = 0; g < G; ++g) order[g] = g;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return w[kProgWords * a + 3] > w[kProgWords * b + 3]; });
    auto shares = [&](int g) {
        int k = 0;
        for (int m = 0; m < B; ++m) k += where(G + m) == where(g);
        return k;
    };
    double sum_busy = 0, sum_scan = 0, sum_busy_m = 0, sum_busy_nm = 0;
    int nm = 0;
    for (int g = 0; g < G; ++g) {
        sum_busy += (double)w[kProgWords * g + 3];
        sum_scan += (double)w[kProgWords * g + 2];
        if (shares(g)) { sum_busy_m += (double)w[kProgWords * g + 3]; ++nm; } else sum_busy_nm += (double)w[kProgWords * g + 3];
    }
    fprintf(stderr, "persist wg busy (ms, 100 MHz ticks): mean scan %.2f busy %.2f | with a merger on the CU (%d WGs) %.2f, "
                    "without %.2f | slowest:",
            sum_scan / G * 1e-5, sum_busy / G * 1e-5, nm, nm ? sum_busy_m / nm * 1e-5 : 0.0,
            G > nm ? sum_busy_nm / (G - nm) * 1e-5 : 0.0);
    for (int k = 0; k < 8 && k < G; ++k) {
        const int g = order[k];
        fprintf(stderr, " #%d(scan %.2f busy %.2f xcc %u se %u cu %u mergers %d)", g, w[kProgWords * g + 2] * 1e-5,
                w[kProgWords * g + 3] * 1e-5, (where(g) >> 8) & 0xf, (where(g) >> 4) & 0xf, where(g) & 0xf, shares(g));
    }
    fprintf(stderr, " | fastest: #%d(busy %.2f)\n", order[G - 1], w[kProgWords * order[G - 1] + 3] * 1e-5);
}

// After a persistent wait timed out: which workgroups are furthest behind, in which phase, on which XCD/SE/CU,
// and what their last wait saw (PersistArgs::prog).
static std::string progress_summary(ksched_ctx *c) {
    if (!c->d_prog) return "";
    const int n = c->prog_G + c->prog_B + kCommitWGs;
    std::vector<uint64_t> w((size_t)kProgWords * n);
    if (hipMemcpy(w.data(), c->d_prog, w.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return "";
    const Ctl *h = reinterpret_cast<const Ctl *>(c->h_cursor);
    std::string out = "; polls satisfied by the atomic read " + std::to_string(h->polls_rmw);
    auto group = [&](const char *name, int lo, int hi) {
        int64_t bmin = INT64_MAX, bmax = -1;
        for (int i = lo; i < hi; ++i) {
            const int64_t b = (int64_t)(w[kProgWords * i] >> 8);
            bmin = std::min(bmin, b); bmax = std::max(bmax, b);
        }
        char t[160];
        snprintf(t, sizeof t, "; %s batches %lld..%lld", name, (long long)bmin, (long long)bmax);
        out += t;
        int shown = 0;
        for (int i = lo; i < hi && shown < 6; ++i) {
            if ((int64_t)(w[kProgWords * i] >> 8) != bmin || bmin == bmax) continue;
            const uint32_t where = (uint32_t)(w[kProgWords * i + 1] >> 32);
            snprintf(t, sizeof t, " [#%d phase %#x xcc %u se %u cu %u saw %llu polls %llu]", i - lo,
                     (unsigned)(w[kProgWords * i] & 0xff), (where >> 8) & 0xf, (where >> 4) & 0xf, where & 0xf,
                     (unsigned long long)(w[kProgWords * i + 1] & 0xffffffffull),
                     (unsigned long long)w[kProgWords * i + 2]);
            out += t;
            if (i < c->prog_G && w[kProgWords * i + 4]) {
                out += " waves";
                for (int v = 0; v < 8; ++v) {
                    const uint64_t x = w[kProgWords * i + 4 + v];
                    snprintf(t, sizeof t, " %lld:%#x", (long long)(x >> 8), (unsigned)(x & 0xff));
                    out += t;
                }
            }
            ++shown;
        }
    };
    group("score", 0, c->prog_G);
    group("merge", c->prog_G, c->prog_G + c->prog_B);
    group("commit", c->prog_G + c->prog_B, n);
    for (int i = c->prog_G + c->prog_B; i < n; ++i) {
        const uint32_t where = (uint32_t)(w[kProgWords * i + 1] >> 32);
        char t[160];
        snprintf(t, sizeof t, "; commit workgroup %d: batch %lld phase %#x on xcc %u se %u cu %u", i - c->prog_G - c->prog_B,
                 (long long)(w[kProgWords * i] >> 8), (unsigned)(w[kProgWords * i] & 0xff), (where >> 8) & 0xf,
                 (where >> 4) & 0xf, where & 0xf);
        out += t;
    }
    return out;
}

// The device error word of the call that just finished, as the call's error.
int decode_device_error(ksched_ctx *c, int32_t e) {
    if (e == 0) return KSCHED_OK;
    const int nprog = c->prog_G + c->prog_B + kCommitWGs;
    auto cleared = [&](const std::string &msg) {  // (the exact kernels clear the word before every launch)
        (void)hipMemsetAsync(c->d->err, 0, sizeof(int32_t), c->stream);
        return fail(c, KSCHED_E_DEVICE, msg);
    };
    auto wait = [&](const std::string &what) {  // a wait of the persistent pipeline timed out
        const Ctl *h = reinterpret_cast<const Ctl *>(c->h_cursor);
        char buf[400];
        snprintf(buf, sizeof buf,
                 "persistent pipeline: %s timed out (committed %llu, arrive %llu/%llu/%llu/%llu, merged "
                 "%llu/%llu/%llu/%llu, cursor %lld, merger-0 batches %lld, rank %d/%d)",
                 what.c_str(), h->committed, h->arrive[0].v, h->arrive[1].v, h->arrive[2].v, h->arrive[3].v, h->merged[0].v,
                 h->merged[1].v, h->merged[2].v, h->merged[3].v, (long long)h->cursor, (long long)h->nact, c->o.rank,
                 c->o.nranks);
        return cleared(std::string(buf) + progress_summary(c));
    };
    switch (e) {
        case kErrWaitMerged: return wait("the commit's wait for the merges");
        case kErrWaitCommit: return wait("a score or merger workgroup's wait for commit(b-" + std::to_string(kPipeLag) + ")");
        case kErrWaitArrive: return wait("a merger's wait for the score workgroups");
        case kErrScorePlan: return wait("the score grid's plan (idle)");
        case kErrCommitPlan: return wait("the commit's plan (idle)");
        case kErrWaitPeerLists: return wait("a merger's wait for a peer rank's candidate lists (node-sharded exchange)");
        case kErrRankBarrier: return wait("the ranks' device barrier (node-sharded exchange)");
        case kErrStreamMergeWait: return cleared("batched mode: the merge's wait for the score workgroups timed out");
        case kErrStreamScoreWait: return cleared("batched mode: the score's wait for commit(b-2) timed out");
        case kErrLdsCanary: {
            std::vector<uint64_t> w((size_t)nprog * kProgWords);
            uint64_t where = 0;
            if (!w.empty() && hipMemcpy(w.data(), c->d_prog, w.size() * 8, hipMemcpyDeviceToHost) == hipSuccess)
                for (int i = c->prog_G + c->prog_B; i < c->prog_G + c->prog_B + 2; ++i) where |= w[(size_t)kProgWords * i + 2];
            char buf[200];
            snprintf(buf, sizeof buf, "persistent pipeline: the commit's LDS canary changed (batch %llu, word %llu, low bits %#llx)",
                     (unsigned long long)(where >> 32), (unsigned long long)((where >> 16) & 0xffff),
                     (unsigned long long)(where & 0xffff));
            return cleared(buf);
        }
        case kErrBadIndex: {
            std::vector<uint64_t> w((size_t)nprog * kProgWords);
            uint64_t d = 0, v = 0;
            if (hipMemcpy(w.data(), c->d_prog, w.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
                d = w[(size_t)kProgWords * (c->prog_G + c->prog_B) + 3];
                v = w[(size_t)kProgWords * (c->prog_G + c->prog_B) + 4];
            }
            char buf[240];
            snprintf(buf, sizeof buf, "persistent pipeline: the commit produced a node index outside every node (%#llx; batch %llu, "
                     "pod lane %llu, path %llu; a device protocol error, results discarded)", (unsigned long long)v,
                     (unsigned long long)(d >> 40), (unsigned long long)((d >> 32) & 0xff), (unsigned long long)(d & 0xffffffffu));
            return cleared(buf);
        }
        case kErrWaitRescue: return cleared("persistent pipeline: the commit's wait for a rescue timed out");
        default:  // kErrExactExchange
            return fail(c, KSCHED_E_DEVICE, "exact mode: cross-workgroup exchange timed out (workgroups not co-resident?)");
    }
}

}  // namespace ksched

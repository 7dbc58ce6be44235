// ksched_kernels.hip -- the utility kernels and their launchers: node-row upkeep (k_prep_nodes, k_apply_delta), a
// batched call's control block (k_ctl_init), one pod's FailedScheduling reasons (k_explain), system-scope zeroing
// (k_zero_sys), the division self-test (k_selftest_div).  The pipelines and modes have units of their own.  Compiled
// with -ffp-contract=off: every double op rounds individually, exactly like the Go reference.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ksched_kernels.h"

namespace ksched {

// (re)derive af / y of every node row from its int64 allocatable
__global__ void k_prep_nodes(NodeRec *nodes, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    NodeRec *nd = nodes + i;
    set_node(nd, nd->a[0], nd->a[1], nd->a[2]);
}

// Pipeline control at the start of a batched call: batch 0 starts at pod 0, batch 1 speculatively at B;
// every later plan is written by the commit two batches earlier (plan_after_commit).
__global__ void k_ctl_init(Ctl *ctl, int B, int64_t P, int lag) {
    if (threadIdx.x != 0) return;
    ctl->cursor = 0; ctl->spec_next = 0; ctl->resync = 0;
    for (int i = 0; i < 5; ++i) ctl->stats[i] = 0;
    ctl->scored = 0;
    ctl->committed = 0;
    for (int i = 0; i < 4; ++i) { ctl->arrive[i].v = 0; ctl->merged[i].v = 0; ctl->inh_done[i].v = 0; }
    for (int i = 0; i < kCtlReplicas; ++i) ctl->committed_x[i].v = 0;
    ctl->rescue_req.v = 0;
    ctl->rescue_done.v = 0;
    for (int i = 0; i < 16; ++i) (&ctl->hrec.v)[i] = 0;  // (v and pad: the two hand-off granules)
    ctl->polls_rmw = 0;
    for (int i = 0; i < kPlanRing; ++i) ctl->cursor_at[i] = 0;
    ctl->nact = 0;
    for (int i = 0; i < kPlanRing; ++i) ctl->plan[i] = -1;
    // the first `lag` plans (batch b's commit plans batch b + lag)
    for (int i = 0; i < lag; ++i) ctl->plan[i] = (int64_t)i * B < P ? (int64_t)i * B : -1;
}

__global__ void k_apply_delta(NodeRec *nodes, int64_t n, int64_t k, const int32_t *idx, const int64_t *d) {
    // Sequential in one lane: deltas may repeat a node and must apply in order (wrapping adds).
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int64_t i = 0; i < k; ++i) {
        const int64_t j = idx[i];
        if (j < 0 || j >= n) continue;
        NodeRec *nd = nodes + j;
        set_node(nd, (int64_t)((uint64_t)nd->a[0] + (uint64_t)d[i]), (int64_t)((uint64_t)nd->a[1] + (uint64_t)d[k + i]),
                 (int64_t)((uint64_t)nd->a[2] + (uint64_t)d[2 * k + i]));
    }
}

// FailedScheduling reasons of one pod against the current node state (anchor/predicate.go:134-148,
// the failures list of :157): per node the FIRST failing check in the reference's order -- CPU,
// Memory, Pod -- then the build-defined label check; 0 = fits.  Lane = node, coalesced u8 stores,
// per-wave ballot counts folded with one vector atomic per reason per wave.
__global__ void k_explain(const NodeRec *nodes, int64_t n, int64_t rc, int64_t rm, int64_t rp, uint64_t sel,
                          int use_labels, uint8_t *reason, unsigned long long *counts) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int r = -1;
    if (j < n) {
        const NodeRec &nd = nodes[j];
        r = nd.a[0] < rc ? 1 : nd.a[1] < rm ? 2 : nd.a[2] < rp ? 3 : (use_labels && (nd.labels & sel) != sel) ? 4 : 0;
        if (reason) reason[j] = (uint8_t)r;
    }
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < kNumReasons; ++k) {
        const unsigned long long m = __ballot(r == k);
        if (lane == 0 && m) atomicAdd(counts + k, (unsigned long long)__popcll(m));
    }
}

__global__ void k_selftest_div(int64_t n, const double *a, const double *b, double *native, double *fast) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i], y = b[i];
    native[i] = x / y;
    fast[i] = qdiv(x, y, recip(y));
}

__global__ void k_zero_sys(uint64_t *p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        __hip_atomic_store(p + i, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
hipError_t launch_prep_nodes(NodeRec *nodes, int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_prep_nodes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, nodes, n);
    return hipGetLastError();
}

hipError_t launch_apply_delta(NodeRec *nodes, int64_t n, int64_t k, const int32_t *idx, const int64_t *d,
                              hipStream_t s) {
    hipLaunchKernelGGL(k_apply_delta, dim3(1), dim3(64), 0, s, nodes, n, k, idx, d);
    return hipGetLastError();
}

hipError_t launch_explain(const NodeRec *nodes, int64_t n, int64_t rc, int64_t rm, int64_t rp, uint64_t sel,
                          bool use_labels, uint8_t *reason, unsigned long long *counts, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_explain, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, nodes, n, rc, rm, rp, sel,
                       (int)use_labels, reason, counts);
    return hipGetLastError();
}

hipError_t launch_ctl_init(Ctl *ctl, int B, int64_t P, int lag, hipStream_t s) {
    hipLaunchKernelGGL(k_ctl_init, dim3(1), dim3(64), 0, s, ctl, B, P, lag);
    return hipGetLastError();
}

hipError_t launch_zero_sys(void *p, size_t bytes, hipStream_t s) {
    const int64_t n = (int64_t)(bytes / 8);
    if (n <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(k_zero_sys, dim3((unsigned)blocks), dim3(256), 0, s, static_cast<uint64_t *>(p), n);
    return hipGetLastError();
}

hipError_t launch_selftest_div(int64_t n, const double *a, const double *b, double *native, double *fast,
                               hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_selftest_div, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, a, b, native, fast);
    return hipGetLastError();
}

}  // namespace ksched

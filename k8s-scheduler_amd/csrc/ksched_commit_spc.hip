// ksched_commit_spc.hip -- the stream pipeline's speculative commit kernel: commit_spc_batch (ksched_commit.h, shared
// with the persistent pipeline's commit workgroups), 30 instantiations built in parallel with ksched_stream.hip.
#include <hip/hip_runtime.h>

#include "ksched_commit.h"
#include "ksched_stream.h"

namespace ksched {

// <= 192 VGPRs (amdgpu_num_vgpr counts half the unified gfx950 file): beside a resident score
// workgroup (two 64-VGPR waves per SIMD) the commit's two waves per SIMD must fit the 512-entry file,
// or a score grid polling for this commit would never let it in.
template <int K, int PRIO, int DOM, bool LAB, bool F53>
__global__ __launch_bounds__(kSpcThreads) __attribute__((amdgpu_num_vgpr(96))) void k_commit_spc(CommitArgs A) {
    __builtin_amdgcn_s_setprio(3);  // latency-critical: win issue arbitration over co-resident score waves
    extern __shared__ __attribute__((aligned(16))) char smem[];
    commit_spc_batch<K, PRIO, DOM, LAB, F53, false>(A, smem);
}

namespace {
template <int PRIO, int DOM, bool LAB, bool F53>
StreamKernel commit_spc_k(int K) {
    switch (K) {
        case 4: return {(const void *)k_commit_spc<4, PRIO, DOM, LAB, F53>, spc_lds_bytes<4>()};
        case 8: return {(const void *)k_commit_spc<8, PRIO, DOM, LAB, F53>, spc_lds_bytes<8>()};
        case 16: return {(const void *)k_commit_spc<16, PRIO, DOM, LAB, F53>, spc_lds_bytes<16>()};
        default: return {};
    }
}
}  // namespace

StreamKernel commit_spc_kernel(int K, int prio, int dom, bool lab, bool f53) {
    KSCHED_DISPATCH(prio, dom, lab, f53, (commit_spc_k<P_, D_, L_, F_>(K)));
}

hipError_t launch_commit_spc(int K, int prio, int dom, bool lab, bool f53, const CommitArgs &a, hipStream_t s) {
    if (a.B > 64) return hipErrorInvalidValue;
    const StreamKernel k = commit_spc_kernel(K, prio, dom, lab, f53);
    return launch_stream_kernel(k, dim3(1), dim3(kSpcThreads), &a, k.lds, s);
}

}  // namespace ksched

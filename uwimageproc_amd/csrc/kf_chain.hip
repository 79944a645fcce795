// The key-frame chain's walker on the device: one lane runs kf_chain.hpp's walk() between the matcher rounds of a pipe
// step.  Its state and the rows it writes are plain stores to global memory; the next kernel on the stream reads them.
#include "uwip_internal.hpp"

namespace {
__global__ __launch_bounds__(64) void k_kf_chain(uwip_kf::Batch b, uwip_kf::State *state, uwip_kf::Bufs u, int round)
{
    if (threadIdx.x != 0) return;
    uwip_kf::State s = *state;
    uwip_kf::walk(b, s, u, round);
    *state = s;
}
}  // namespace

int uwip_kf_walk(uwip_ctx *ctx, const uwip_kf::Batch &b, uwip_kf::State *d_state, const uwip_kf::Bufs &u, int round)
{
    uwip_kscope ks(ctx, "k_kf_chain");
    k_kf_chain<<<1, 64, 0, ctx->stream>>>(b, d_state, u, round);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}

// The device side of uwip_pipe_step_streams (include/uwip.h, "compressed frames in, compressed key frames out"): what lies
// between the decoders, the four stages and the encoders of a step that never waits for the host.  DESIGN.md 7c.
//   k_ps_blank      zero the frames of the decoded batch whose decoder status is negative (read on the device);
//   k_ps_select     one small block: the list of frames this step emits -- the good frames (UWIP_EMIT_ALL) or the rows the
//                   key-frame walker wrote to the ring during this step (UWIP_EMIT_KEYFRAMES: ring[emitted .. total), `emitted`
//                   being the pipe's device-side count of rows already handed out) -- as (source, stream index, row ID) and a
//                   count.  A source < F is a frame of this batch, F the carried frame;
//   k_ps_gather     copy the listed frames into a compact batch of F + 1 frames (more rows cannot close in one step);
//   k_ps_carry      after the gather: the enhanced pixels of the walker's carry_best slot go to the pipe's carried frame, as
//                   k_kf_slot_copy carries that slot's features;
//   (the encoders run on the compact batch with the list's length as their device count)
//   k_ps_table      one block: exclusive scan of the non-negative sizes, the table of outs, the statuses, ratios and aclahe
//                   parameters next to it;
//   k_ps_pack       copy the streams out of their slots into one contiguous blob.
// The copies use 16-byte stores wherever the destination allows and 16-byte loads where the source is aligned alike; the head
// and tail of a range, and a source that is not, go byte by byte.
#include "uwip_internal.hpp"
#include "pipe_streams.hpp"

namespace {

using uwip_ps::Sel;
using uwip_ps::TableHdr;

// zero [dst, dst + n) by the threads tid, tid + nthr, ...
__device__ __forceinline__ void ps_zero(uint8_t *__restrict__ dst, size_t n, size_t tid, size_t nthr)
{
    size_t head = (size_t)(16 - ((uintptr_t)dst & 15)) & 15;
    if (head > n) head = n;
    const size_t nvec = (n - head) / 16, tail0 = head + nvec * 16;
    for (size_t i = tid; i < head; i += nthr) dst[i] = 0;
    uint4 *v = reinterpret_cast<uint4 *>(dst + head);
    for (size_t i = tid; i < nvec; i += nthr) v[i] = make_uint4(0u, 0u, 0u, 0u);
    for (size_t i = tail0 + tid; i < n; i += nthr) dst[i] = 0;
}

// copy [src, src + n) to [dst, dst + n) (no overlap) by the threads tid, tid + nthr, ...
__device__ __forceinline__ void ps_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, size_t n, size_t tid, size_t nthr)
{
    size_t head = (size_t)(16 - ((uintptr_t)dst & 15)) & 15;
    if (head > n) head = n;
    const size_t nvec = (n - head) / 16, tail0 = head + nvec * 16;
    for (size_t i = tid; i < head; i += nthr) dst[i] = src[i];
    uint4 *dv = reinterpret_cast<uint4 *>(dst + head);
    if ((((uintptr_t)(src + head)) & 15) == 0) {
        const uint4 *sv = reinterpret_cast<const uint4 *>(src + head);
        for (size_t i = tid; i < nvec; i += nthr) dv[i] = sv[i];
    } else {
        // the source is not aligned like the destination: its bytes one by one, the store still 16 bytes wide
        for (size_t i = tid; i < nvec; i += nthr) {
            const uint8_t *s = src + head + i * 16;
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = (uint32_t)s[4 * k] | ((uint32_t)s[4 * k + 1] << 8) | ((uint32_t)s[4 * k + 2] << 16) | ((uint32_t)s[4 * k + 3] << 24);
            dv[i] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    for (size_t i = tail0 + tid; i < n; i += nthr) dst[i] = src[i];
}

// grid (x, F): frame blockIdx.y is zeroed when its status is negative
__global__ __launch_bounds__(256) void k_ps_blank(uint8_t *__restrict__ frames, size_t frame_bytes, const int32_t *__restrict__ status)
{
    const int f = blockIdx.y;
    if (status[f] >= 0) return;
    ps_zero(frames + (size_t)f * frame_bytes, frame_bytes, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

// one block.  emit_all: the good frames among the first `valid`; else the rows ring[*emitted .. *total) of the walker, a row
// whose stream index lies in [base, base + F) naming that frame of this batch, any other the carried frame (source F).
__global__ __launch_bounds__(64) void k_ps_select(int emit_all, int F, int valid, int base, const int32_t *__restrict__ status,
                                                  const uwip_keyframe_row *__restrict__ ring, int max_rows,
                                                  const uint32_t *__restrict__ total, uint32_t *__restrict__ emitted,
                                                  Sel *__restrict__ sel, int32_t *__restrict__ sel_n)
{
    if (threadIdx.x != 0) return;
    int n = 0;
    if (emit_all) {
        for (int f = 0; f < valid; ++f)
            if (status[f] >= 0) { sel[n].src = f; sel[n].index = base + f; sel[n].row_id = -1; sel[n].pad = 0; ++n; }
    } else {
        const uint32_t t = *total;
        uint32_t e = *emitted;
        if (t - e > (uint32_t)max_rows) e = t - (uint32_t)max_rows;         // rows a raw step left behind and the ring has lost
        for (; e != t && n < F + 1; ++e) {
            const uwip_keyframe_row r = ring[e % (uint32_t)max_rows];
            const bool here = r.index >= base && r.index - base < F;
            sel[n].src = here ? r.index - base : F;
            sel[n].index = r.index; sel[n].row_id = r.id; sel[n].pad = 0;
            ++n;
        }
        *emitted = t;
    }
    *sel_n = n;
}

// grid (x, F + 1): entry blockIdx.y of the list goes to frame blockIdx.y of the compact batch
__global__ __launch_bounds__(256) void k_ps_gather(const uint8_t *__restrict__ work, const uint8_t *__restrict__ carried, int F,
                                                   size_t frame_bytes, const Sel *__restrict__ sel, const int32_t *__restrict__ sel_n,
                                                   uint8_t *__restrict__ compact)
{
    const int e = blockIdx.y;
    if (e >= *sel_n) return;
    const int s = sel[e].src;
    if (s < 0 || s > F) return;
    const uint8_t *from = s < F ? work + (size_t)s * frame_bytes : carried;
    ps_copy(compact + (size_t)e * frame_bytes, from, frame_bytes, (size_t)blockIdx.x * blockDim.x + threadIdx.x,
            (size_t)gridDim.x * blockDim.x);
}

// grid (x): the frame in the walker's carry_best slot (1 + frame; < 1: nothing to carry) becomes the carried frame
__global__ __launch_bounds__(256) void k_ps_carry(const uint8_t *__restrict__ work, int F, size_t frame_bytes,
                                                  const int32_t *__restrict__ carry_best, uint8_t *__restrict__ carried)
{
    const int slot = *carry_best;
    if (slot < 1 || slot > F) return;
    ps_copy(carried, work + (size_t)(slot - 1) * frame_bytes, frame_bytes, (size_t)blockIdx.x * blockDim.x + threadIdx.x,
            (size_t)gridDim.x * blockDim.x);
}

// one block of 256: the table of a result.  Exclusive scan of max(size, 0) over the list: every thread sums a contiguous share
// of the entries, the shares' sums are scanned through LDS (64 bits: a step's blob may pass 4 GiB).
__global__ __launch_bounds__(256) void k_ps_table(int F, const Sel *__restrict__ sel, const int32_t *__restrict__ sel_n,
                                                  const int64_t *__restrict__ sizes, const int32_t *__restrict__ status,
                                                  const float *__restrict__ ratio, const int32_t *__restrict__ par,
                                                  TableHdr *__restrict__ hdr, uwip_stream_out *__restrict__ outs,
                                                  int32_t *__restrict__ t_status, float *__restrict__ t_ratio, int32_t *__restrict__ t_par)
{
    __shared__ uint64_t s_part[256];
    const int t = threadIdx.x;
    int n = *sel_n;
    if (n > F + 1) n = F + 1;
    const int per = (n + 255) / 256, e0 = min(t * per, n), e1 = min(e0 + per, n);
    uint64_t sum = 0;
    for (int e = e0; e < e1; ++e) sum += sizes[e] > 0 ? (uint64_t)sizes[e] : 0u;
    s_part[t] = sum;
    __syncthreads();
    uint64_t off = 0;
    for (int j = 0; j < t; ++j) off += s_part[j];
    for (int e = e0; e < e1; ++e) {
        uwip_stream_out o;
        o.index = sel[e].index; o.row_id = sel[e].row_id; o.size = sizes[e]; o.offset = (int64_t)off;
        outs[e] = o;
        off += sizes[e] > 0 ? (uint64_t)sizes[e] : 0u;
    }
    if (t == 255) { hdr->n_outs = n; hdr->reserved = 0; hdr->blob_bytes = off; }
    // par: the aclahe stage's [F][4] record (BS, CL, ..) where the choice was made on the device, else null (the host has it)
    for (int f = t; f < F; f += 256) {
        t_status[f] = status[f]; t_ratio[f] = ratio[f];
        t_par[2 * f] = par ? par[4 * f] : 0; t_par[2 * f + 1] = par ? par[4 * f + 1] : 0;
    }
}

// grid (x, F + 1): stream blockIdx.y leaves its slot for its place in the blob
__global__ __launch_bounds__(256) void k_ps_pack(const uint8_t *__restrict__ slots, size_t slot_bytes, const TableHdr *__restrict__ hdr,
                                                 const uwip_stream_out *__restrict__ outs, uint8_t *__restrict__ blob)
{
    const int e = blockIdx.y;
    if (e >= hdr->n_outs) return;
    const uwip_stream_out o = outs[e];
    if (o.size <= 0 || (uint64_t)o.size > (uint64_t)slot_bytes) return;
    ps_copy(blob + o.offset, slots + (size_t)e * slot_bytes, (size_t)o.size, (size_t)blockIdx.x * blockDim.x + threadIdx.x,
            (size_t)gridDim.x * blockDim.x);
}

}  // namespace

namespace {
// workgroups along x for a range of `bytes`: 16 KiB per workgroup and pass, at most 64 of them per frame
unsigned copy_blocks(size_t bytes) { return (unsigned)std::min<size_t>(64, std::max<size_t>(1, (bytes + 16383) / 16384)); }
}  // namespace

int uwip_ps_blank(uwip_ctx *ctx, uint8_t *d_frames, int F, size_t frame_bytes, const int32_t *d_status)
{
    uwip_kscope ks(ctx, "k_ps_blank");
    k_ps_blank<<<dim3(copy_blocks(frame_bytes), F), 256, 0, ctx->stream>>>(d_frames, frame_bytes, d_status);
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}

int uwip_ps_select_gather(uwip_ctx *ctx, const uwip_ps::Step &s)
{
    {
        uwip_kscope ks(ctx, "k_ps_select");
        k_ps_select<<<1, 64, 0, ctx->stream>>>(s.emit_all, s.F, s.valid, s.base, s.status, s.ring, s.max_rows, s.total, s.emitted, s.sel,
                                               s.sel_n);
    }
    {
        uwip_kscope ks(ctx, "k_ps_gather");
        k_ps_gather<<<dim3(copy_blocks(s.frame_bytes), s.F + 1), 256, 0, ctx->stream>>>(s.work, s.carried, s.F, s.frame_bytes, s.sel, s.sel_n,
                                                                                        s.compact);
    }
    if (s.carry_best) {
        uwip_kscope ks(ctx, "k_ps_carry");
        k_ps_carry<<<copy_blocks(s.frame_bytes), 256, 0, ctx->stream>>>(s.work, s.F, s.frame_bytes, s.carry_best, s.carried);
    }
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}

int uwip_ps_pack(uwip_ctx *ctx, const uwip_ps::Step &s, const int64_t *d_sizes, const float *d_ratio, const int32_t *d_par,
                 const uint8_t *d_slots, size_t slot_bytes, uint8_t *d_table, uint8_t *d_blob)
{
    TableHdr *hdr = reinterpret_cast<TableHdr *>(d_table);
    uwip_stream_out *outs = reinterpret_cast<uwip_stream_out *>(d_table + uwip_ps::outs_offset());
    {
        uwip_kscope ks(ctx, "k_ps_table");
        k_ps_table<<<1, 256, 0, ctx->stream>>>(s.F, s.sel, s.sel_n, d_sizes, s.status, d_ratio, d_par, hdr, outs,
                                               reinterpret_cast<int32_t *>(d_table + uwip_ps::status_offset(s.F)),
                                               reinterpret_cast<float *>(d_table + uwip_ps::ratio_offset(s.F)),
                                               reinterpret_cast<int32_t *>(d_table + uwip_ps::par_offset(s.F)));
    }
    {
        uwip_kscope ks(ctx, "k_ps_pack");
        k_ps_pack<<<dim3(copy_blocks(slot_bytes), s.F + 1), 256, 0, ctx->stream>>>(d_slots, slot_bytes, hdr, outs, d_blob);
    }
    UWIP_HIP(ctx, hipGetLastError());
    return UWIP_OK;
}

// What pipe.cpp (the host side of uwip_pipe_step_streams) and pipe_streams.hip (its kernels) share.  Plain C++: the emulated
// test includes it with the host compiler.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/uwip.h"

namespace uwip_ps {

// one entry of the list k_ps_select writes: which frame (0..F-1 of this batch, F = the carried frame), its stream index, the
// key-frame row's ID (-1 under UWIP_EMIT_ALL)
struct Sel { int32_t src, index, row_id, pad; };

// A result's table in device memory, copied to the host in one piece: header, outs [F + 1], statuses [F], ratios [F], the aclahe
// stage's (BS, CL) [F][2].
struct TableHdr { int32_t n_outs, reserved; uint64_t blob_bytes; };
inline size_t outs_offset() { return sizeof(TableHdr); }
inline size_t status_offset(int F) { return outs_offset() + sizeof(uwip_stream_out) * ((size_t)F + 1); }
inline size_t ratio_offset(int F) { return status_offset(F) + sizeof(int32_t) * (size_t)F; }
inline size_t par_offset(int F) { return ratio_offset(F) + sizeof(float) * (size_t)F; }
inline size_t table_bytes(int F) { return par_offset(F) + 2 * sizeof(int32_t) * (size_t)F; }

// everything the selection kernels of one step read and write (device pointers)
struct Step {
    int emit_all, F, valid, base, max_rows;
    size_t frame_bytes;
    const int32_t *status;              // [F] the decoders' statuses
    const uwip_keyframe_row *ring;      // key-frame mode: the walker's row ring, its row count, its carry_best slot
    const uint32_t *total;
    const int32_t *carry_best;          // null under UWIP_EMIT_ALL: nothing is carried
    uint32_t *emitted;                  // rows already handed out
    const uint8_t *work;                // [F] the enhanced frames
    uint8_t *carried, *compact;         // one frame; [F + 1] frames
    Sel *sel;
    int32_t *sel_n;
};

}  // namespace uwip_ps

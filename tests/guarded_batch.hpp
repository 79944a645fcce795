// A strided, misaligned batch of n frames between guard bytes, for the decoder harnesses (jpeg_decode_emulated.cpp,
// png_decode_emulated.cpp): rows padded by 5 bytes, frames by 77, the base pointer off by 3, every byte 0xA5 before the call.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "uwip.h"
struct Batch {
    std::vector<uint8_t> buf;
    uwip_batch_u8 b;
    Batch(int n, int rows, int cols, int channels)
    {
        std::memset(&b, 0, sizeof b);
        b.rows = rows; b.cols = cols; b.channels = channels; b.frames = n;
        b.step = (size_t)cols * channels + 5; b.frame_stride = b.step * rows + 77;
        buf.assign(b.frame_stride * n + 3, 0xA5);
        b.data = buf.data() + 3;
    }
    const uint8_t *row(int f, int y) const { return buf.data() + 3 + f * b.frame_stride + y * b.step; }
    bool clean() const                                         // nothing but the frames' rows was written
    {
        for (size_t i = 0; i < buf.size(); ++i) {
            const size_t o = i < 3 ? SIZE_MAX : (i - 3) % b.frame_stride;
            const bool inside = o != SIZE_MAX && o / b.step < (size_t)b.rows && o % b.step < (size_t)b.cols * b.channels;
            if (!inside && buf[i] != 0xA5) return false;
        }
        return true;
    }
};

// icl_ws_layout.h -- the places of a workspace's pieces inside one allocation: a bump allocator over offsets.  Plain host arithmetic
// with no HIP in it (tests/ws_layout_main.cpp compiles it with the host compiler alone).
#pragma once
#include <cstddef>

struct icl_ws_layout {
    size_t align; // every piece starts on a multiple of it (a power of two is not required)
    size_t total = 0; // bytes taken so far: the next piece's offset, and at the end what the allocation must hold
    explicit icl_ws_layout(size_t alignment) : align(alignment) {}
    // The offset of a piece of `bytes` bytes.  The piece occupies its size rounded up to the alignment: a piece of 0 bytes takes no room
    // (its offset is the next piece's), and pieces taken one after the other are one contiguous range.
    size_t take(size_t bytes)
    {
        const size_t at = total;
        total += (bytes + align - 1) / align * align;
        return at;
    }
};

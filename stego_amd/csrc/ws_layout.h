// A workspace carved into regions, written once: plan() takes the regions in order and keeps their offsets, the launcher turns an
// offset into a typed pointer with at<T>().  take(bytes, align) rounds the running offset up to `align` (a power of two), returns it as
// the region's offset and advances by `bytes`; total(align) is the rounded size of everything taken.  Both styles in use are this:
// every region on its own 16 bytes (take(n, 16) ... total(16)), and regions packed tight with only the size rounded (take(n, 1) ...
// total(8)).  Plain C++17, no HIP types: tests/test_ws_layout_host.py compiles this header alone with g++.
#pragma once
#include <cstddef>

namespace stego {

struct WsLayout {
    size_t off = 0;

    static size_t round_up(size_t v, size_t align) { return (v + align - 1) & ~(align - 1); }

    size_t take(size_t bytes, size_t align)
    {
        const size_t at = round_up(off, align);
        off = at + bytes;
        return at;
    }

    size_t total(size_t align) const { return round_up(off, align); }
};

// the region at byte offset `off` of the workspace `ws`
template <class T>
inline T* at(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }

}  // namespace stego

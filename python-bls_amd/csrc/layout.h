// layout.h -- the one helper every workspace of the host side is laid out with (plain C++, no HIP).
#pragma once
#include <stddef.h>

namespace ws {

// consecutive arrays in one buffer, each rounded up to `unit` (a power of two: 256 bytes in the byte workspaces, 4 words in the
// sums' word workspaces, 64 words in the folded table, 1 where the arrays are packed); `off` is the running offset and, at the
// end, the size
struct Layout {
    size_t unit, off;
    size_t take(size_t count) { const size_t o = off; off += (count + unit - 1) & ~(unit - 1); return o; }
};

}   // namespace ws

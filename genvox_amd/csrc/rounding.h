// The two roundings of every layout in the tree.  Plain C++ and no device: the host-arithmetic headers that stand-alone programs and
// CPU tests include (disc_conv.h, the *_internal.h) use it as the .hip files do.
#pragma once
#include <cstddef>

namespace gvx {
inline size_t round64(size_t floats) { return (floats + 63) & ~(size_t)63; }    // every tensor of a blob starts on 256 bytes
inline size_t round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }  // ... and every region of a workspace, features buffer or tape
}  // namespace gvx

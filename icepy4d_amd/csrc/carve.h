// Host arithmetic of the stage entry points: 1-D grid sizes, and the layout of one scratch buffer as consecutive 256-byte-aligned
// pieces. Nothing of HIP in here: tests/carve_host_harness.cpp compiles it with a plain host compiler.
#pragma once
#include <cstddef>

namespace im {

inline long long blocks_of(long long n, int per) { return (n + per - 1) / per; }
inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

// Two phases over one buffer. First every piece is taken, in order: `auto a = c.take<T>(count)` reserves up256(count * sizeof(T)) bytes
// behind the pieces before it, and c.bytes is then what the buffer must hold (ctx->grow). Once the buffer is there, a.at(base) is the piece.
struct Carve {
    template <typename T> struct Piece {
        size_t offset;
        T* at(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + offset); }
    };
    size_t bytes = 0;
    template <typename T> Piece<T> take(size_t count) {
        const Piece<T> p{bytes};
        bytes += up256(count * sizeof(T));
        return p;
    }
};

}  // namespace im

// Workspace carving of the decoder block drivers (lm_block.cpp, t5_block.cpp).  A driver has ONE layout function: it takes buffers from an
// Arena in a fixed order.  On a null base the arena only counts - that run is the driver's *_workspace_bytes - and on the caller's workspace
// the same run hands out the pointers, so the size a caller is told and the offsets the driver uses cannot disagree.
#ifndef EAVQA_BLOCK_WS_H
#define EAVQA_BLOCK_WS_H
#include <stddef.h>

namespace eavqa_block {
inline size_t align_up(size_t v) { return (v + 255) & ~size_t(255); }

struct Arena {
    char* base;
    size_t used = 0;
    explicit Arena(void* workspace) : base(static_cast<char*>(workspace)) {}
    template <class T = void> T* take(size_t bytes) {
        T* p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += align_up(bytes);
        return p;
    }
};
}
#endif

// Layout of the one temporary device buffer a host-buffer entry point stages its images through (csrc/hjr_device_internal.h: HostStage).
// Plain C++, no HIP: tests/native/stage_layout_test.cpp runs it on the host.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

namespace hjr {
struct StageLayout {
    // One staged image: `slot` is the caller's device-pointer variable, `src` the host image uploaded ahead of the launch (null: none), `dst`
    // the host image downloaded behind it (null: none); neither = scratch.
    struct Item { void* slot; const void* src; void* dst; size_t bytes, off; };
    std::vector<Item> items;
    size_t at = 0;
    // The cursor: offsets front to back.  `align` is a power of two, at least 4; a zero-byte request returns the current aligned offset and
    // moves nothing (the image behind it may start at the same offset: a zero-byte image is never addressed).
    size_t take(size_t bytes, size_t align)
    {
        const size_t o = (at + align - 1) & ~(align - 1);
        if (bytes) at = o + bytes;
        return o;
    }
    size_t total() const { return at; }
    template <class T> void add(T*& d, const void* src, void* dst, size_t bytes, size_t align) { items.push_back({ &d, src, dst, bytes, take(bytes, align) }); }
    // every slot = base + its offset (all object pointers have one representation here)
    void resolve(void* base) const
    {
        for (const Item& it : items) {
            char* const p = static_cast<char*>(base) + it.off;
            memcpy(it.slot, &p, sizeof(p));
        }
    }
};
} // namespace hjr

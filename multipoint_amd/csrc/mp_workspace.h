// Carving a caller-owned workspace into typed arrays (host code).  Every feature has ONE function X_workspace(base, shape...)
// that takes its arrays from a Carver in a fixed order and returns them with the total: called on nullptr it is the size the
// public sizer reports, called on the caller's pointer it is where the launches write.  The size and the layout cannot drift
// apart, because there is no second statement of either.
#pragma once
#include <cstddef>

struct Carver {
    char* base;
    size_t at = 0;
    size_t align = 256;            // every array starts on a multiple of this (a power of two; 1: packed)

    explicit Carver(void* base_, size_t align_ = 256) : base(static_cast<char*>(base_)), align(align_) {}

    // `count` elements of T at the current position (nullptr when only the size is asked for)
    template <class T> T* take(size_t count)
    {
        T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;
        at += (count * sizeof(T) + align - 1) & ~(align - 1);
        return p;
    }
    size_t bytes() const { return at; }
};

// The layout of a scratch buffer, stated once: a buffer (device memory, or its host image) is a sequence of typed regions, and
// the calls that carve one address it through the spans its Layout hands out, never through byte offsets of their own.
//   * regions lie in the order of the add() calls;
//   * every region starts at a multiple of max(16, alignof(T)): the kernels' 16-byte accesses are safe on any of them;
//   * a zero count gives an empty span, which takes no room;
//   * bytes() is the end of the last region, rounded up to 16.
// A run of consecutive regions, "a to b", is the bytes [a.offset, b.end()) (run_bytes): what one copy moves.  A host image is a
// std::vector<uint8_t> of Layout::bytes(), addressed through the same spans.  Host-only, plain C++17.
#pragma once
#include <cstdint>

namespace pgo {

template <class T>
struct Span {
  int64_t offset = 0, count = 0;
  T* in(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + offset); }
  const T* in(const void* base) const { return reinterpret_cast<const T*>(static_cast<const char*>(base) + offset); }
  int64_t bytes() const { return count * (int64_t)sizeof(T); }
  int64_t end() const { return offset + bytes(); }
};

template <class A, class B>
int64_t run_bytes(const Span<A>& a, const Span<B>& b) {
  return b.end() - a.offset;
}

class Layout {
 public:
  template <class T>
  Span<T> add(int64_t count) {
    constexpr int64_t align = alignof(T) > 16 ? (int64_t)alignof(T) : 16;
    Span<T> s;
    s.offset = (end_ + align - 1) / align * align;
    s.count = count > 0 ? count : 0;
    if (s.count) end_ = s.end();
    return s;
  }
  int64_t bytes() const { return (end_ + 15) / 16 * 16; }

 private:
  int64_t end_ = 0;
};

// a device buffer that is grown on demand and kept (pgo_handle::reserve)
struct Scratch {
  void* p = nullptr;
  int64_t cap = 0;
};

}  // namespace pgo

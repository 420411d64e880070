// Which arrays live in a block of scratch, how big and where, for every entry that takes scratch and for the forward's
// workspace: a family names its arrays once, in a function of take() calls that runs twice, on a plan without a base
// for the size (plan_bytes) and on a plan over the caller's pointer to bind them.
#pragma once
#include <algorithm>
#include <cstddef>

namespace sepvad {
struct ScratchPlan {
  char* base;    // null: the size pass, no pointer is written
  size_t align;  // every array starts on a multiple of it (256; 8 for the families packed as plain doubles)
  size_t off = 0, top = 0;
  explicit ScratchPlan(void* base_ = nullptr, size_t align_ = 256) : base((char*)base_), align(align_) {}
  // p = the next array: `count` elements and `slack` bytes. An empty one (overlay) shares the address of the next.
  template <class T>
  void take(T*& p, size_t count, size_t slack = 0) {
    if (base) p = reinterpret_cast<T*>(base + off);
    off += (count * sizeof(T) + slack + align - 1) / align * align;
    top = std::max(top, off);
  }
  template <class T>
  void overlay(T*& p) { take(p, 0); }
  void rewind() { off = 0; }  // a second phase reuses the same bytes
  size_t bytes() const { return top; }
};
// The size pass of a family's list: list(p) names its arrays on the plan p
template <class L>
long long plan_bytes(L&& list, size_t align = 256) {
  ScratchPlan p(nullptr, align);
  list(p);
  return (long long)p.bytes();
}
}  // namespace sepvad

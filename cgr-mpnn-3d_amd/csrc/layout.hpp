// Regions of a caller-provided buffer (arena, workspace, image buffer, conv scratch) and the one
// placer that lays them out.  A layout is a function that states each region once, as a call on a
// Placer: the member it fills, its element count and whether it exists; everything else -- byte
// offset, typed pointer, total bytes, the answer to a public name query -- derives from that call.
#pragma once

#include <stddef.h>
#include <string.h>

#include <algorithm>

namespace cgr {

constexpr size_t kAlign = 256;
constexpr size_t kNone = (size_t)-1;

// One region: `count` elements of T at byte offset `off` (untyped regions count bytes).  Absent
// until a placer places it; p is set only when the placer was given the buffer.
template <class T>
struct Reg {
  size_t off = kNone;
  size_t count = 0;
  T* p = nullptr;
  operator T*() const { return p; }
};
template <class T>
constexpr size_t reg_elem_bytes = sizeof(T);
template <>
inline constexpr size_t reg_elem_bytes<void> = 1;

// What a placer tells about each named region.  Views are placed with NoNames (nothing on the
// launch path reads a name); the public offset queries place with FindName.
struct NoNames {
  void operator()(const char*, int, size_t) {}
};
struct FindName {
  const char* name;
  int index;
  long long found = -1;
  void operator()(const char* n, int i, size_t off) {
    if (n && strcmp(n, name) == 0 && (i < 0 || i == index)) found = (long long)off;
  }
};

template <class Note = NoNames>
struct Placer {
  char* base = nullptr;  // nullptr: offsets and counts only
  Note note{};
  size_t off = 0;  // bytes placed so far: the buffer's size once every region is stated

  // r when `present`: count elements, the next region kAlign-aligned
  template <class T>
  void operator()(Reg<T>& r, size_t count, bool present = true) {
    if (present) put(r, count, count, kAlign);
  }
  // ... answering the public query `name` (`index`: the entry of an indexed name)
  template <class T>
  void operator()(const char* name, Reg<T>& r, size_t count, bool present = true,
                  int index = -1) {
    (*this)(r, count, present);
    if (present) note(name, index, r.off);
  }
  // `n` layers of `per` elements back to back in one region; the query's index picks the layer
  template <class T>
  void layers(const char* name, Reg<T>& r, size_t per, int n) {
    put(r, per * (size_t)n, per * (size_t)n, kAlign);
    for (int l = 0; l < n; ++l) note(name, l, r.off + (size_t)l * per * reg_elem_bytes<T>);
  }
  // a region whose bytes never shrink below one element; count stays the capacity to check
  template <class T>
  void floored(Reg<T>& r, size_t count) {
    put(r, count, std::max<size_t>(count, 1), kAlign);
  }
  // back to back with the next region (no rounding): the members of a block
  template <class T>
  void packed(Reg<T>& r, size_t count, const char* name = nullptr) {
    put(r, count, count, 1);
    note(name, -1, r.off);
  }
  // the block over the packed members from `first` on, a multiple of `unit` bytes; ends it
  template <class T>
  void block(Reg<void>& r, const Reg<T>& first, size_t unit) {
    r.off = first.off;
    r.p = first.p;
    r.count = (off - first.off + unit - 1) / unit * unit;
    off = (first.off + r.count + kAlign - 1) / kAlign * kAlign;
  }

 private:
  template <class T>
  void put(Reg<T>& r, size_t count, size_t taken, size_t align) {
    r.off = off;
    r.count = count;
    r.p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off = (off + taken * reg_elem_bytes<T> + align - 1) / align * align;
  }
};

}  // namespace cgr

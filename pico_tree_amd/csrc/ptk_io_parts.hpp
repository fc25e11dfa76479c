// ptk_io_parts.hpp -- where the parts of a host-buffer call lie inside a device block, written once.  A call names its
// input parts (queries, radii, values) and its output parts (rows, counts, frames, moments) as two lists; each list is
// laid out in one block of the handle (host_form in ptk_backend.hip, host_form64 in ptk_backend_f64.hpp).
//   - every part begins on a 16-byte boundary (the widest load of a kernel);
//   - an absent optional part -- a null host pointer -- takes no room, moves no other part and has no device pointer;
//   - total() is the end of the last present part rounded up to 16 bytes: what the block must hold at least.
// Plain C++17: no HIP, no handle types, nothing allocated (tests/cpp/io_parts_main.cpp includes nothing else).
#pragma once

#include <cassert>
#include <cstddef>
#include <initializer_list>

namespace ptkio {

constexpr size_t kAlign = 16;
constexpr int kMaxParts = 3;  // aggregate_within: the values, the queries and the radii go up

struct Part {
  const void* host;  // null: the part is absent (whatever `bytes` says)
  size_t bytes;
  bool clear_first;  // an output part whose records have bytes no kernel writes: the block is zeroed before the search
};
inline Part in_part(const void* host, size_t bytes) { return Part{host, bytes, false}; }
inline Part out_part(void* host, size_t bytes, bool clear_first = false) { return Part{host, bytes, clear_first}; }

class Parts {
 public:
  Parts(std::initializer_list<Part> list) {
    assert(list.size() <= (size_t)kMaxParts);
    for (const Part& p : list) {
      part_[n_] = Part{p.host, p.host != nullptr ? p.bytes : 0, p.clear_first};
      offset_[n_] = total_;
      total_ += (part_[n_].bytes + kAlign - 1) & ~(kAlign - 1);
      ++n_;
    }
  }
  int size() const { return n_; }
  bool any() const {  // is any part present?  (none: the call needs no block at all)
    for (int i = 0; i < n_; ++i)
      if (present(i)) return true;
    return false;
  }
  bool present(int i) const { return part_[i].host != nullptr; }
  bool clear_first(int i) const { return part_[i].clear_first; }
  size_t bytes(int i) const { return part_[i].bytes; }
  size_t offset(int i) const { return offset_[i]; }
  size_t total() const { return total_; }
  const void* source(int i) const { return part_[i].host; }                    // of an input part
  void* destination(int i) const { return const_cast<void*>(part_[i].host); }  // of an output part (made by out_part)
  // The device pointer of part i in the block at `base`; null for an absent part.
  template <class T>
  T* at(char* base, int i) const {
    return present(i) ? reinterpret_cast<T*>(base + offset_[i]) : nullptr;
  }

 private:
  Part part_[kMaxParts] = {};
  size_t offset_[kMaxParts] = {};
  size_t total_ = 0;
  int n_ = 0;
};

}  // namespace ptkio

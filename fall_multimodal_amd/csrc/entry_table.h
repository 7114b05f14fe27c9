// The state_dict table of the side nets (f3_targcn, f3_sktr, f3_musa): one entry per parameter, buffer
// and counter in the reference module's order, with its offset into the flat array of its kind.
// net.cpp keeps a table of its own (phase-1 parameters first, offsets finalised late).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "fall3.h"

namespace f3 {

struct EntryTable {
  struct Entry {
    std::string name;
    int kind;
    std::vector<int64_t> shape;
    int64_t off;
  };
  std::vector<Entry> entries;
  int64_t nparam = 0, nbuf = 0, ncnt = 0;

  // Appends an entry and returns its offset: floats for parameters (each entry 16-B aligned, float4
  // RMSprop) and buffers, int64 slots for counters.
  int64_t add(const std::string& name, std::vector<int64_t> shape, int kind = F3_ENTRY_PARAM) {
    int64_t n = 1;
    for (auto d : shape) n *= d;
    Entry e{name, kind, shape, 0};
    if (kind == F3_ENTRY_PARAM) {
      e.off = nparam;
      nparam += (n + 3) / 4 * 4;
    } else if (kind == F3_ENTRY_BUFFER) {
      e.off = nbuf;
      nbuf += n;
    } else {
      e.off = ncnt;
      ncnt += 1;
    }
    entries.push_back(e);
    return e.off;
  }

  int get(int i, const char** name, int* kind, int* ndim, int64_t* shape8, int64_t* offset) const {
    if (i < 0 || i >= (int)entries.size()) return F3_EINVAL;
    const Entry& e = entries[i];
    *name = e.name.c_str();
    *kind = e.kind;
    *ndim = (int)e.shape.size();
    for (int d = 0; d < 8; ++d) shape8[d] = d < (int)e.shape.size() ? e.shape[d] : 0;
    *offset = e.off;
    return F3_OK;
  }
};

}  // namespace f3

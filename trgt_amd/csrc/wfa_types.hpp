// trgt_amd/csrc/wfa_types.hpp -- the records the WFA kernels and the host-side launch plan (wfa_plan.hpp) share.  Plain C++: no HIP here.
#pragma once
#include <cstdint>

namespace trgt {

struct JobDev {  // one alignment: pattern / text inside pat_base / txt_base, output slots
  uint64_t pat_off, txt_off, cigar_off, ops_off;
  uint32_t pat_len, txt_len, out_index, pad;
};

namespace wfa {

constexpr int RING = 32;                      // LDS mirror depth of wavefront descriptors (>= max_score_scope)

struct WfDesc { int lo, hi, lo_alloc; uint32_t base; };  // base == NOBASE: wavefront pointer is NULL; lo > hi: ->null

struct Pen { int metric, x, o1, e1, o2, e2, scope, ncomp; };

}  // namespace wfa
}  // namespace trgt

// The host half of the indexed Merkle tree (include/zkhip.h, "indexed Merkle tree"): the LINKING of a batch of insertions.  The reference finds
// the low leaf of one insertion by a scan over every leaf (`update_idx_leaf`, /root/reference/aggregator/src/utils.rs:101-197); here the used
// values live in an ordered map, so a batch of B insertions costs B log(used) comparisons.  No HIP call anywhere: zkhip_imt_link runs this in a
// process that never initialises a device, and the tree object (capi.hip) runs the same code.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>
#include "../../include/zkhip.hpp"

namespace zkhip {

struct imt_key {                       // a canonical integer, compared from the top word down
  uint64_t w[4];
  bool operator<(const imt_key& o) const {
    for (int i = 3; i >= 0; i--) if (w[i] != o.w[i]) return w[i] < o.w[i];
    return false;
  }
};

// what the linking says about one insertion: the low leaf and the successor the low leaf pointed at BEFORE the insertion (0, 0 past the largest)
struct imt_link {
  uint32_t low, next_idx;
  halo2::Fr low_val, next_val;         // Montgomery
};

class imt_index {
  std::map<imt_key, uint32_t> by_val;  // canonical val -> leaf index; 0 -> 0, the permanent head, is always there
  std::vector<halo2::Fr> vals;         // Montgomery val of every used leaf, by index

  static imt_key canon(const uint64_t mont[4]) {
    const uint64_t raw_one[4] = {1, 0, 0, 0};
    imt_key k;
    halo2::detail::mont_mul(k.w, mont, raw_one, halo2::detail::R_MOD, halo2::detail::R_INV);
    return k;
  }

 public:
  imt_index() {
    by_val[imt_key{{0, 0, 0, 0}}] = 0;
    vals.push_back(halo2::Fr{{0, 0, 0, 0}});
  }
  size_t used() const { return vals.size(); }                       // the head included: also the first free index

  // The insertions of new_vals (n_new x 4 Montgomery words) in order, the first at leaf used(), into a tree of `capacity` leaves.  All or nothing:
  // false leaves the index as it was, *first_bad the first value that is not a canonical word set, is 0, is already in the tree or earlier
  // in the batch, or finds no free leaf; *why says which.  out (nullable): one record per insertion.
  bool link(const uint64_t* new_vals, size_t n_new, size_t capacity, imt_link* out, size_t* first_bad, const char** why) {
    const size_t used0 = vals.size();
    size_t i = 0;
    const char* bad = nullptr;
    for (; i < n_new; i++) {
      const uint64_t* v = new_vals + 4 * i;
      if (used0 + i >= capacity) { bad = "no free leaf is left"; break; }
      if (halo2::detail::geq(v, halo2::detail::R_MOD)) { bad = "not a reduced Montgomery element"; break; }
      const imt_key k = canon(v);
      if (!(k.w[0] | k.w[1] | k.w[2] | k.w[3])) { bad = "the value 0 is the head's"; break; }
      auto it = by_val.lower_bound(k);                              // the successor, or the value itself
      if (it != by_val.end() && !(k < it->first)) { bad = "the value is already in the tree or earlier in the batch"; break; }
      if (out) {
        imt_link& o = out[i];
        if (it != by_val.end()) { o.next_idx = it->second; o.next_val = vals[it->second]; }
        else { o.next_idx = 0; o.next_val = halo2::Fr{{0, 0, 0, 0}}; }
        auto lo = it;
        --lo;                                                       // exists: the head is below every k > 0
        o.low = lo->second;
        o.low_val = vals[lo->second];
      }
      by_val.emplace_hint(it, k, (uint32_t)(used0 + i));
      halo2::Fr m;
      std::memcpy(m.l, v, 32);
      vals.push_back(m);
    }
    if (!bad) return true;
    for (size_t j = 0; j < i; j++) by_val.erase(canon(new_vals + 4 * j));
    vals.resize(used0);
    if (first_bad) *first_bad = i;
    if (why) *why = bad;
    return false;
  }
  void unlink(size_t n) {                                           // takes the last n insertions back (a call that failed after its linking)
    for (size_t j = 0; j < n; j++) { by_val.erase(canon(vals.back().l)); vals.pop_back(); }
  }
};

}  // namespace zkhip

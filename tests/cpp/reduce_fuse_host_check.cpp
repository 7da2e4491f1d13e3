// csrc/reduce_fuse.hpp on the host (tests/test_reduce_fuse_host.py builds this with ASan + UBSan): whether steps 1 and 2 of the reduction
// plan go in one launch, for every window size c = 2 .. 21 and the bucket-set counts of reduce_plan_host_check.cpp.  The program checks that
// a fused pair is the plan's first two entries, adjacent REDUCE_STEP entries with N >= 8 (one pair, so disjoint and in order by itself), that
// the fused launch's strides are the state sizes at step 1 and behind step 2, that its first and last lanes read and write inside B elements,
// that the plan itself is left as it was, and the two plans the shipped thresholds are set for; it prints one line per (c, WB) for the test
// to compare with its restatement in Python:
//   c WB fused lanes
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "reduce_fuse.hpp"

using namespace zkhip;

#define CHECK(cond)                                                                                     \
  do {                                                                                                  \
    if (!(cond)) { fprintf(stderr, "c = %d, WB = %d: failed: %s (line %d)\n", c, WB, #cond, __LINE__); return 1; } \
  } while (0)

static int check_one(int c, int WB) {
  const uint32_t B = 1u << (c - 1);
  reduce_plan* p = (reduce_plan*)calloc(1, sizeof(reduce_plan));
  reduce_plan* before = (reduce_plan*)calloc(1, sizeof(reduce_plan));
  if (!p || !before) return 2;
  CHECK(reduce_make_plan(B, WB, p));
  memcpy(before, p, sizeof(reduce_plan));
  const bool fused = reduce_fuse_first_pair(*p, WB);
  CHECK(memcmp(before, p, sizeof(reduce_plan)) == 0);               // the plan keeps describing single steps
  size_t lanes = 0;
  if (fused) {
    CHECK(p->n >= 2);
    const reduce_launch &L = p->l[0], &L2 = p->l[1];
    CHECK(L.kind == REDUCE_STEP && L2.kind == REDUCE_STEP && L.steps == 1 && L2.steps == 1);     // adjacent single-lane entries
    CHECK(L.s == 1 && L2.s == 2 && L.N == B && L2.N == B / 2 && L.N >= 8);
    CHECK(L.in_stride == reduce_state_elems(L.N, 1) && L.in_stride == B);                          // reads the buckets
    CHECK(L2.out_stride == reduce_state_elems(L.N / 4, 3) && L2.out_stride == L.N / 4 + 2 * (L.N / 8));   // writes the state before step 3
    CHECK(L2.out_stride <= B);
    CHECK((L.N / 4) % 2 == 0);                                        // both lanes of a pair exist
    for (uint32_t t : {0u, 1u, L.N / 4 - 2, L.N / 4 - 1}) {           // the first and the last lane pair: reads X[4t .. 4t+3], writes X''[t] and one Z element
      CHECK(4 * t + 3 < L.in_stride);
      CHECK(t < L.N / 4 && L.N / 4 + (t & 1 ? L.N / 8 : 0) + t / 2 < L2.out_stride);
    }
    CHECK(L.N / 4 + (L.N / 4 - 2) / 2 < L.N / 4 + L.N / 8);           // row Z''^0 ends where Z''^1 begins
    lanes = (size_t)(L.N / 4) * WB;
    CHECK(lanes >= REDUCE_FUSE_MIN_LANES && lanes < REDUCE_FUSE_END_LANES);
  }
  if (c == 20 && WB == 1) CHECK(fused && lanes == ((size_t)1 << 17));  // (2^19, 1): steps 1 + 2, as shipped
  if (c == 18 && WB == 1) CHECK(!fused);                              // (2^17, 1): one single-lane entry, nothing to fuse
  printf("%d %d %d %zu\n", c, WB, fused ? 1 : 0, lanes);
  free(p); free(before);
  return 0;
}

int main() {
  const int sets[] = {1, 2, 5, 8, 13, 16, 43, 63, 64, 65, 100, 2048, 2049, 65535};
  int cases = 0;
  for (int c = 2; c <= 21; c++)
    for (int WB : sets) {
      if ((uint64_t)WB << (c - 1) >= (1ull << 31)) continue;      // msm_build_tasks refuses these
      const int rc = check_one(c, WB);
      if (rc) return rc;
      cases++;
    }
  printf("reduce fuse host check done: %d cases\n", cases);
  return 0;
}

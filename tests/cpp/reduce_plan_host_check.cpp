// csrc/reduce_plan.hpp on the host (tests/test_reduce_plan_host.py builds this with ASan + UBSan): the launch plan of the bucket reduction
// for every window size c = 2 .. 21 and a range of bucket-set counts.  The program checks the plan's own invariants -- the launches consume
// steps 1 .. c-2 exactly once and in order, every launch's input stride is its predecessor's output stride and the size of the state at its
// step, no launch reads or writes past a ping-pong buffer of B elements, the finish kernel's levels fit its LDS buffers and its quads -- and
// prints each plan, one line per (c, WB), for the test to compare with its restatement in Python:
//   c WB finish nz last_stride  kind s steps N in_stride out_stride  ...
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "reduce_plan.hpp"

using namespace zkhip;

#define CHECK(cond)                                                                                     \
  do {                                                                                                  \
    if (!(cond)) { fprintf(stderr, "c = %d, WB = %d: failed: %s (line %d)\n", c, WB, #cond, __LINE__); return 1; } \
  } while (0)

static int check_one(int c, int WB) {
  const uint32_t B = 1u << (c - 1);
  reduce_plan* p = (reduce_plan*)malloc(sizeof(reduce_plan));     // on the heap: the sanitizer sees a write past l[]
  if (!p) return 2;
  CHECK(reduce_make_plan(B, WB, p));
  CHECK(p->n >= (p->finish ? 1 : 0) && p->n <= REDUCE_MAX_LAUNCHES);
  CHECK(p->finish == (WB <= REDUCE_FINISH_MAX_SETS));
  CHECK(p->nz == (c >= 2 ? c - 2 : 0));
  int s = 1;
  uint32_t N = B, stride = B;
  for (int i = 0; i < p->n; i++) {
    const reduce_launch& L = p->l[i];
    CHECK(L.s == s && L.N == N && L.N == (B >> (s - 1)));         // steps in order, none twice, none skipped
    CHECK(L.in_stride == stride && stride == reduce_state_elems(N, s) && stride <= B);     // strides chain and are the state's size
    if (L.kind == REDUCE_FINISH) {
      CHECK(i == p->n - 1 && p->finish);
      CHECK(L.steps == (c - 2) - (s - 1) && L.steps >= 0);
      uint32_t M = N;
      for (int k = 0, t = s; M > 2; k++, t++, M >>= 1) {
        const uint32_t adds = reduce_step_adds(M, t);
        CHECK(adds <= (k % 2 == 0 ? REDUCE_FINISH_ADDS : REDUCE_FINISH_ADDS2));           // every level fits the LDS buffer of its parity
        CHECK(M + (uint32_t)(t - 1) * (M / 2) <= (k == 0 ? B : (k % 2 == 1 ? REDUCE_FINISH_ADDS : REDUCE_FINISH_ADDS2)));   // and reads inside its input
      }
      CHECK(M == 2);
      s += L.steps;
      N = 2;
      continue;
    }
    CHECK(L.kind == REDUCE_STEP || L.kind == REDUCE_STEP_QUAD || L.kind == REDUCE_PAIR_QUAD);
    CHECK(L.steps == (L.kind == REDUCE_PAIR_QUAD ? 2 : 1));
    CHECK(N > 2 && (L.steps == 1 || N >= 8));
    const uint32_t adds = reduce_step_adds(N, s);
    if (L.kind == REDUCE_STEP) CHECK((size_t)adds * WB > REDUCE_QUAD_MAX);
    else CHECK((size_t)adds * WB <= REDUCE_QUAD_MAX);
    if (L.kind == REDUCE_PAIR_QUAD) {
      CHECK(L.out_stride == reduce_step_adds(N / 2, s + 1));
      CHECK((size_t)L.out_stride * WB * 8 < REDUCE_PAIR_MAX_LANES);
    } else CHECK(L.out_stride == adds);
    CHECK(L.out_stride <= B && L.out_stride == reduce_state_elems(N >> L.steps, s + L.steps));
    stride = L.out_stride;
    N >>= L.steps;
    s += L.steps;
  }
  CHECK(s - 1 == p->nz);                       // steps 1 .. c-2, each once
  CHECK(N == 2 && (p->finish || stride == p->last_stride));
  if (!p->finish) CHECK(p->last_stride == (uint32_t)(2 + p->nz));
  printf("%d %d %d %d %u", c, WB, p->finish ? 1 : 0, p->nz, p->last_stride);
  for (int i = 0; i < p->n; i++) printf("  %d %d %d %u %u %u", p->l[i].kind, p->l[i].s, p->l[i].steps, p->l[i].N, p->l[i].in_stride, p->l[i].out_stride);
  printf("\n");
  free(p);
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
  printf("reduce plan host check done: %d cases\n", cases);
  return 0;
}

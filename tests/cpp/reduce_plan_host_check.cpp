// csrc/reduce_plan.hpp on the host (tests/test_reduce_plan_host.py builds this with ASan + UBSan): the launch plan of the bucket reduction
// for every window size c = 2 .. 21, a range of bucket-set counts and both kinds of bases.  The program checks the plan's own invariants
// -- the launches consume steps 1 .. c-2 exactly once and in order, every launch's input stride is its predecessor's output stride and the
// size of the state at its step, no launch reads or writes past a ping-pong buffer of B elements, the finish kernel's levels fit its LDS
// buffers and its quads, a fused pair is the first launch, has N >= 8 and an even N / 4 and a lane count inside its window, one
// weighted-sum launch follows the pyramid and a store or a fold follows it exactly where it does not write the results --, executes the plan
// on integers with the index maps the kernels use (below), and prints each plan, one line per (c, WB, prepared), for the test to compare
// with its restatement in Python:
//   c WB prepared finish direct nz last_stride  kind s steps N in_stride out_stride grid  ...
//
// The model: one bucket set of seeded uint64_t values b_k; an addition wraps, a doubling is x 2.  Every entry is applied the way its kernel
// applies the shared operand functions, each state in a heap buffer of exactly in_stride / out_stride elements (the finish kernel's LDS
// buffers: REDUCE_FINISH_ADDS and REDUCE_FINISH_ADDS2 elements), so the sanitizer sees every lane's reads and writes; the result must be
// sum_k (k + 1) b_k mod 2^64.  One set is enough: sets differ only by an offset.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "reduce_plan.hpp"

using namespace zkhip;

#define CHECK(cond)                                                                                     \
  do {                                                                                                  \
    if (!(cond)) { fprintf(stderr, "c = %d, WB = %d, prepared = %d: failed: %s (line %d)\n", c, WB, (int)prepared, #cond, __LINE__); return 1; } \
  } while (0)

struct state {                       // exactly n elements on the heap
  uint64_t* p;
  uint32_t n;
  explicit state(uint32_t n_) : p((uint64_t*)malloc((size_t)n_ * sizeof(uint64_t))), n(n_) {}
  ~state() { free(p); }
  state(const state&) = delete;
  state& operator=(const state&) = delete;
};

// one pyramid step as k_pyramid_step, k_pyramid_step_quad and a level of k_reduce_finish run it: one addition per output element
static void model_step(const uint64_t* in, uint64_t* out, uint32_t N, int s) {
  const uint32_t per_win = reduce_step_adds(N, s);
  for (uint32_t t = 0; t < per_win; t++) {
    uint32_t ia, ib;
    reduce_step_operands(N, s, t, ia, ib);
    out[t] = in[ia] + in[ib];
  }
}

// k_pyramid_pair_quad: two pair sums per output, added
static void model_pair_quad(const uint64_t* in, uint64_t* out, uint32_t N, int s) {
  const uint32_t outs = N / 4 + (uint32_t)(s + 1) * (N / 8);
  for (uint32_t o = 0; o < outs; o++) {
    uint64_t pair[2];
    for (uint32_t half = 0; half < 2; half++) {
      uint32_t ia, ib;
      reduce_pair_quad_operands(N, s, o, half, ia, ib);
      pair[half] = in[ia] + in[ib];
    }
    out[o] = pair[0] + pair[1];
  }
}

// k_pyramid_pair: lane pairs (t, t ^ 1) exchange one value
static void model_pair(const uint64_t* in, uint64_t* out, uint32_t N) {
  for (uint32_t t = 0; t < N / 4; t += 2) {
    uint64_t z[2], b[2];
    for (uint32_t k = 0; k < 2; k++) {
      const uint32_t lane = t + k;
      const uint64_t p3 = in[reduce_pair_in(lane, 3)], p1 = in[reduce_pair_in(lane, 1)];
      z[k] = p1 + p3;
      const uint64_t a = in[reduce_pair_in(lane, 0)] + p1;
      b[k] = in[reduce_pair_in(lane, 2)] + p3;
      out[reduce_pair_x_out(lane)] = a + b[k];
    }
    out[reduce_pair_z_out(N, t)] = z[0] + z[1];           // the even lane receives z(2v+1)
    out[reduce_pair_z_out(N, t + 1)] = b[0] + b[1];       // the odd one b(2v)
  }
}

// final state [X0, X1, Z^0 .. Z^(nz-1)]: X0 + X1 + sum_l 2^l Z^l + 2^nz X1
static uint64_t model_weighted_sum(const uint64_t* st, int nz) {
  uint64_t r = st[0] + st[1] + (st[1] << nz);
  for (int l = 0; l < nz; l++) r += st[2 + l] << l;
  return r;
}

// k_reduce_finish: the first level reads the state, the later ones ping-pong between the two LDS buffers
static uint64_t model_finish(const uint64_t* in, uint32_t N, int s) {
  if (N <= 2) return model_weighted_sum(in, s - 1);
  state lds0(REDUCE_FINISH_ADDS), lds1(REDUCE_FINISH_ADDS2);
  const uint64_t* cur = in;
  bool first = true;
  while (N > 2) {
    uint64_t* nxt = first ? lds0.p : (cur == lds0.p ? lds1.p : lds0.p);
    model_step(cur, nxt, N, s);
    cur = nxt; first = false;
    N >>= 1;
    s++;
  }
  return model_weighted_sum(cur, s - 1);
}

static int check_one(int c, int WB, bool prepared) {
  const uint32_t B = 1u << (c - 1);
  reduce_plan* p = (reduce_plan*)malloc(sizeof(reduce_plan));     // on the heap: the sanitizer sees a write past l[]
  if (!p) return 2;
  CHECK(reduce_make_plan(B, WB, prepared, p));
  CHECK(p->n >= 1 && p->n <= REDUCE_MAX_LAUNCHES);
  CHECK(p->finish == (WB <= REDUCE_FINISH_MAX_SETS));
  CHECK(p->direct == (prepared && WB <= REDUCE_HORNER_QUAD_MAX_SETS));
  CHECK(p->nz == (c >= 2 ? c - 2 : 0));
  int s = 1, sums = 0, tails = 0;
  uint32_t N = B, stride = B;
  bool fused = false;
  size_t lanes = 0;
  // the model's buckets and their weighted sum
  state* cur = new state(B);
  uint64_t want = 0, got = 0, x = 0x9E3779B97F4A7C15ull * (uint64_t)(c * 131 + 7) + (uint64_t)WB;
  for (uint32_t k = 0; k < B; k++) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;                      // xorshift64
    cur->p[k] = x;
    want += (uint64_t)(k + 1) * x;
  }
  for (int i = 0; i < p->n; i++) {
    const reduce_launch& L = p->l[i];
    if (L.kind == REDUCE_STORE || L.kind == REDUCE_FOLD) {          // behind the weighted sum, where that did not write the results
      CHECK(i == p->n - 1 && sums == 1 && !p->direct);
      CHECK(L.kind == (prepared ? REDUCE_STORE : REDUCE_FOLD));
      CHECK(L.grid == (prepared ? ((uint32_t)WB + STORE_THREADS - 1) / STORE_THREADS : 1u) && L.out_stride == 0 && L.steps == 0);
      tails++;
      continue;
    }
    CHECK(sums == 0);                                              // nothing of the pyramid behind the weighted sum
    CHECK(L.s == s && L.N == N && L.N == (B >> (s - 1)));         // steps in order, none twice, none skipped
    CHECK(L.in_stride == stride && stride == reduce_state_elems(N, s) && stride <= B && stride == cur->n);     // strides chain and are the state's size
    if (L.kind == REDUCE_FINISH) {
      CHECK(p->finish && L.grid == (uint32_t)WB && L.out_stride == 0);
      CHECK(L.steps == (c - 2) - (s - 1) && L.steps >= 0);
      uint32_t M = N;
      for (int k = 0, t = s; M > 2; k++, t++, M >>= 1) {
        const uint32_t adds = reduce_step_adds(M, t);
        CHECK(adds <= (k % 2 == 0 ? REDUCE_FINISH_ADDS : REDUCE_FINISH_ADDS2));           // every level fits the LDS buffer of its parity
        CHECK(adds * 4 <= (uint32_t)FINISH_THREADS);                                      // and the workgroup's quads
        CHECK(M + (uint32_t)(t - 1) * (M / 2) <= (k == 0 ? B : (k % 2 == 1 ? REDUCE_FINISH_ADDS : REDUCE_FINISH_ADDS2)));   // and reads inside its input
      }
      CHECK(M == 2);
      got = model_finish(cur->p, N, s);
      s += L.steps;
      N = 2;
      sums++;
      continue;
    }
    if (L.kind == REDUCE_HORNER_QUAD || L.kind == REDUCE_HORNER) {
      CHECK(!p->finish && N == 2 && L.steps == 0 && L.out_stride == 0);
      CHECK(L.kind == (WB <= REDUCE_HORNER_QUAD_MAX_SETS ? REDUCE_HORNER_QUAD : REDUCE_HORNER));
      CHECK(L.grid == (L.kind == REDUCE_HORNER_QUAD ? (uint32_t)WB : ((uint32_t)WB * 32 + HORNER_THREADS - 1) / HORNER_THREADS));
      CHECK((uint64_t)L.grid * (L.kind == REDUCE_HORNER_QUAD ? 1 : HORNER_THREADS / 32) >= (uint64_t)WB);      // a group of lanes per set
      CHECK(p->nz + 2 <= 32 && stride == (uint32_t)(2 + p->nz));                            // one term per lane of a 32-lane group
      got = model_weighted_sum(cur->p, s - 1);
      sums++;
      continue;
    }
    CHECK(L.kind == REDUCE_STEP || L.kind == REDUCE_STEP_QUAD || L.kind == REDUCE_PAIR_QUAD || L.kind == REDUCE_PAIR);
    CHECK(L.steps == (L.kind == REDUCE_PAIR_QUAD || L.kind == REDUCE_PAIR ? 2 : 1));
    CHECK(N > 2 && (L.steps == 1 || N >= 8));
    const uint32_t adds = reduce_step_adds(N, s);
    if (L.kind == REDUCE_STEP || L.kind == REDUCE_PAIR) CHECK((size_t)adds * WB > REDUCE_QUAD_MAX);
    else CHECK((size_t)adds * WB <= REDUCE_QUAD_MAX);
    state* nxt = new state(L.out_stride);
    if (L.kind == REDUCE_PAIR_QUAD) {
      CHECK(L.out_stride == reduce_step_adds(N / 2, s + 1));
      CHECK((size_t)L.out_stride * WB * 8 < REDUCE_PAIR_MAX_LANES);
      CHECK((uint64_t)L.grid * PYRAMID_THREADS >= 8ull * L.out_stride && (uint64_t)(L.grid - 1) * PYRAMID_THREADS < 8ull * L.out_stride);
      model_pair_quad(cur->p, nxt->p, N, s);
    } else if (L.kind == REDUCE_PAIR) {
      CHECK(i == 0 && L.s == 1 && L.N == B && L.N >= 8);                                  // steps 1 and 2: the plan's first launch
      CHECK((size_t)reduce_step_adds(N / 2, 2) * WB > REDUCE_QUAD_MAX);                   // both would be single-lane steps
      CHECK(L.in_stride == reduce_state_elems(L.N, 1) && L.in_stride == B);               // reads the buckets
      CHECK(L.out_stride == reduce_state_elems(L.N / 4, 3) && L.out_stride == L.N / 4 + 2 * (L.N / 8));   // writes the state before step 3
      CHECK((L.N / 4) % 2 == 0);                                                          // both lanes of a pair exist
      CHECK(reduce_pair_z_out(L.N, L.N / 4 - 2) < L.N / 4 + L.N / 8);                     // row Z''^0 ends where Z''^1 begins
      CHECK((uint64_t)L.grid * PYRAMID_THREADS >= L.N / 4 && (uint64_t)(L.grid - 1) * PYRAMID_THREADS < L.N / 4);
      fused = true;
      lanes = (size_t)(L.N / 4) * WB;
      CHECK(lanes >= REDUCE_FUSE_MIN_LANES && lanes < REDUCE_FUSE_END_LANES);
      model_pair(cur->p, nxt->p, N);
    } else {
      CHECK(L.out_stride == adds);
      const uint64_t per = L.kind == REDUCE_STEP ? 1 : 4;                                  // lanes per addition
      CHECK((uint64_t)L.grid * PYRAMID_THREADS >= per * adds && (uint64_t)(L.grid - 1) * PYRAMID_THREADS < per * adds);
      model_step(cur->p, nxt->p, N, s);
    }
    CHECK(L.out_stride <= B && L.out_stride == reduce_state_elems(N >> L.steps, s + L.steps));
    delete cur;
    cur = nxt;
    stride = L.out_stride;
    N >>= L.steps;
    s += L.steps;
  }
  delete cur;
  CHECK(s - 1 == p->nz);                       // steps 1 .. c-2, each once
  CHECK(N == 2 && (p->finish || stride == p->last_stride));
  if (!p->finish) CHECK(p->last_stride == (uint32_t)(2 + p->nz));
  CHECK(sums == 1 && tails == (p->direct ? 0 : 1));
  CHECK(got == want);                          // the plan, executed, is sum_k (k + 1) b_k
  if (c == 20 && WB == 1) CHECK(fused && lanes == ((size_t)1 << 17));  // (2^19, 1): steps 1 + 2, as shipped
  if (c == 18 && WB == 1) CHECK(!fused);                              // (2^17, 1): one single-lane entry, nothing to fuse
  printf("%d %d %d %d %d %d %u", c, WB, prepared ? 1 : 0, p->finish ? 1 : 0, p->direct ? 1 : 0, p->nz, p->last_stride);
  for (int i = 0; i < p->n; i++) printf("  %d %d %d %u %u %u %u", p->l[i].kind, p->l[i].s, p->l[i].steps, p->l[i].N, p->l[i].in_stride, p->l[i].out_stride, p->l[i].grid);
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
      for (int prepared = 0; prepared < 2; prepared++) {
        const int rc = check_one(c, WB, prepared != 0);
        if (rc) return rc;
        cases++;
      }
    }
  printf("reduce plan host check done: %d cases\n", cases);
  return 0;
}

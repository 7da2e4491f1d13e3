// csrc/scan_plan.hpp on the host (tests/test_scan_plan_host.py builds this with ASan + UBSan and supplies the cases): the level plan of the
// chunked scans and the workspace sizes built on it, printed as decimal integers for the test to compare with Python's.
//
// stdin, one case per line: a word and its decimal arguments.  stdout per case, one line:
//   plan N ROW_BYTES                 L  total  n[1] off[1]  ...  n[L] off[L]  n[L + 1]
//   poly N | batch N COUNT | roots N M | perm NPERM CHUNK LOG_N | lookup N_LOOKUPS LOG_N | paillier N N_COLS        the *_workspace_bytes
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "scan_plan.hpp"

using namespace zkhip;

int main() {
  char what[32];
  int cases = 0;
  while (scanf("%30s", what) == 1) {
    const bool plan = !strcmp(what, "plan"), perm = !strcmp(what, "perm"), poly = !strcmp(what, "poly");
    uint64_t a[3] = {0, 0, 0};
    const int want = perm ? 3 : poly ? 1 : 2;
    for (int i = 0; i < want; i++)
      if (scanf("%" SCNu64, &a[i]) != 1) { fprintf(stderr, "bad input line %d\n", cases); return 2; }
    if (plan) {
      const scan_plan p((size_t)a[0], (size_t)a[1]);
      printf("%d %zu", p.L, p.bytes);
      for (int k = 1; k <= p.L; k++) printf(" %zu %zu", p.n[k], p.off[k]);
      printf(" %zu\n", p.n[p.L + 1]);
    } else if (poly) printf("%zu\n", poly_workspace_bytes((size_t)a[0]));
    else if (!strcmp(what, "batch")) printf("%zu\n", poly_batch_workspace_bytes((size_t)a[0], (size_t)a[1]));
    else if (!strcmp(what, "roots")) printf("%zu\n", poly_roots_workspace_bytes((size_t)a[0], (uint32_t)a[1]));
    else if (perm) printf("%zu\n", perm_workspace_bytes((uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2]));
    else if (!strcmp(what, "lookup")) printf("%zu\n", lookup_products_workspace_bytes((uint32_t)a[0], (uint32_t)a[1]));
    else if (!strcmp(what, "paillier")) printf("%zu\n", paillier_tally_workspace_bytes((size_t)a[0], (uint32_t)a[1]));
    else { fprintf(stderr, "bad word on line %d: %s\n", cases, what); return 2; }
    cases++;
  }
  printf("scan plan host check done: %d cases\n", cases);
  return 0;
}

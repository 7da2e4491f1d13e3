// csrc/rowvm_blob.hpp on the host (tests/test_rowvm_blob_host.py builds this with ASan + UBSan): the one blob layout and the one fill of the
// row-program interpreter, for program shapes on both sides of every rounding (the lists below), alone and side by side, around the 2^12
// split of the power tables, over whole columns and over window buffers.  Per case the program checks
//   - the plan: every offset a multiple of 256, the pieces (column table, omega, part records, each region's micro-ops, constants and rotation
//     offsets, the two power tables) pairwise disjoint and inside `total`, the staged prefix ending where the power tables begin;
//   - the fill, into a heap buffer of EXACTLY `staged` bytes (the sanitizer sees a write past it): column table, omega, part records pointing
//     into their own regions, rotation offsets by the rule of their form, constants;
//   - every micro-op, padding no-ops included, under a host model of the kernel's address rule (vm_load_resolved of rowvm.hip)
//         address = base + ((row + off) & wrap & sign-extended mask) * 32
//     for operands a and b at rows 0 and rows - 1: a masked operand lands on the element of the named column the instruction asks for and
//     inside that column's extent (the domain, or halo_lo + count + halo_hi of a window buffer), every other one inside the program's own
//     constants region (a constant: on its 32 bytes);
//   - the operands: those of the instruction, except that a product with exactly one memory operand has it second.
// and prints one line for the test to compare with the byte formulas the two launch paths used before they became one:
//   n_insns n_constants n_rotations n_columns n_progs log_rows mode staged total
// Several programs: the named shape is program n_progs / 2, program j beside it has the shape shape_of() gives (restated in the test).
// Every combination of the lists is a case, except that a launch of 257 programs takes one of the three modes per shape, in turn.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "rowvm_blob.hpp"

using namespace zkhip;

static const uint32_t INSNS[] = {1, 2, 3, 4, 5, 1000}, CONSTS[] = {0, 1, 7, 8, 9}, ROTS[] = {0, 1, 3, 256}, COLUMNS[] = {0, 1, 31, 32, 33}, PROGS[] = {1, 2, 5, 257},
                      LOG_ROWS[] = {0, 11, 12, 13};
enum { MODE_WHOLE = 0, MODE_WHOLE_SCALED = 1, MODE_WINDOW = 2, MODES = 3 };      // whole columns with rot_scale 1 / 4; window buffers with rot_scale 4

#define CHECK(cond)                                                                                                                         \
  do {                                                                                                                                      \
    if (!(cond)) {                                                                                                                          \
      fprintf(stderr, "insns %u consts %u rots %u columns %u progs %u log_rows %u mode %d: failed: %s (line %d)\n", INSNS[ii], CONSTS[ci], ROTS[ri], n_columns, \
              n_progs, log_rows, mode, #cond, __LINE__);                                                                                    \
      return 1;                                                                                                                             \
    }                                                                                                                                       \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;      // xorshift64
  return (uint32_t)((g_rng >> 20) % n);
}

// the shape of program j of a case named by the list indices (ii, ci, ri): the named one in the middle, short ones beside it
static void shape_of(uint32_t n_progs, uint32_t j, int ii, int ci, int ri, uint32_t* n_insns, uint32_t* n_constants, uint32_t* n_rotations) {
  if (j == n_progs / 2) { *n_insns = INSNS[ii]; *n_constants = CONSTS[ci]; *n_rotations = ROTS[ri]; return; }
  *n_insns = INSNS[(ii + j) % 5];
  *n_constants = CONSTS[(ci + j) % 5];
  *n_rotations = ROTS[(ri + j) % 3];
}

struct program {        // a zkhip_vm_program and the arrays it points to
  std::vector<zkhip_vm_insn> insns;
  std::vector<uint64_t> constants;
  std::vector<int32_t> rotations;
};

static zkhip_vm_operand random_operand(uint32_t n_constants, uint32_t n_rotations, uint32_t n_columns, bool rowpow) {
  uint8_t kinds[6];                                                       // what row_vm_validate lets this program name
  uint32_t n = 0;
  kinds[n++] = ZKHIP_SRC_REG;
  kinds[n++] = ZKHIP_SRC_PREV;
  if (n_constants) kinds[n++] = ZKHIP_SRC_CONST;
  if (n_columns && n_rotations) kinds[n++] = ZKHIP_SRC_COLUMN, kinds[n++] = ZKHIP_SRC_COLUMN;
  if (rowpow) kinds[n++] = ZKHIP_SRC_ROWPOW;
  zkhip_vm_operand o;
  o.kind = kinds[rnd(n)];
  o.rot = 0;
  o.index = 0;
  if (o.kind == ZKHIP_SRC_CONST) o.index = (uint16_t)(rnd(2) ? n_constants - 1 : rnd(n_constants));
  if (o.kind == ZKHIP_SRC_REG) o.index = (uint16_t)rnd(VM_MAX_REGS);
  if (o.kind == ZKHIP_SRC_COLUMN) { o.index = (uint16_t)(rnd(2) ? n_columns - 1 : rnd(n_columns)); o.rot = (uint8_t)(rnd(2) ? n_rotations - 1 : rnd(n_rotations)); }
  return o;
}

static bool is_mem(const zkhip_vm_operand& o) { return o.kind == ZKHIP_SRC_COLUMN || o.kind == ZKHIP_SRC_CONST; }

static int check_one(int ii, int ci, int ri, uint32_t n_columns, uint32_t n_progs, uint32_t log_rows, int mode) {
  const bool window = mode == MODE_WINDOW, with_omega = (ii + ci + ri + (int)n_columns) % 3 != 0;
  const uint64_t domain = (uint64_t)1 << log_rows;
  const uint64_t count = log_rows == 0 ? 37 : domain / 2 + 1;        // a window's rows (log_rows = 0: independent rows, as the verifier runs them)
  const uint64_t rows = window ? count : domain, wrap = window ? ~0ull : domain - 1;
  static const uint64_t omega[4] = {0x1122334455667788ull, 2, 3, 4};
  // the programs
  std::vector<program> store(n_progs);
  std::vector<zkhip_vm_program> progs(n_progs);
  for (uint32_t j = 0; j < n_progs; j++) {
    uint32_t n_insns, n_constants, n_rotations;
    shape_of(n_progs, j, ii, ci, ri, &n_insns, &n_constants, &n_rotations);
    program& s = store[j];
    s.constants.resize((size_t)n_constants * 4);
    for (uint64_t& w : s.constants) w = ((uint64_t)rnd(1u << 30) << 20) | j;
    s.rotations.resize(n_rotations);
    for (uint32_t k = 0; k < n_rotations; k++) {
      s.rotations[k] = (int32_t)(k % 2 ? 1 : -1) * (int32_t)((k / 2) % 9 + (k == 0 ? 0 : 1));       // 0, 1, -2, 2, -3, ...: both signs
      if (log_rows == 0 && window) s.rotations[k] = 0;                                              // independent rows name no rotation but 0
      else if (!window && k % 5 == 4) s.rotations[k] = (int32_t)(k % 2 ? 1 : -1) * (int32_t)(domain + 3);   // whole columns: reduced modulo the domain
    }
    s.insns.resize(n_insns);
    for (zkhip_vm_insn& in : s.insns) {
      in.op = (uint8_t)rnd(ZKHIP_OP_MAD + 1);
      in.dst = (uint8_t)rnd(VM_MAX_REGS);
      in.reserved = 0;
      in.a = random_operand(n_constants, n_rotations, n_columns, with_omega);
      in.b = random_operand(n_constants, n_rotations, n_columns, with_omega);
      in.c = random_operand(n_constants, n_rotations, n_columns, with_omega);
    }
    zkhip_vm_program& p = progs[j];
    p.insns = s.insns.data(); p.n_insns = n_insns;
    p.constants = n_constants ? s.constants.data() : nullptr; p.n_constants = n_constants;
    p.rotations = n_rotations ? s.rotations.data() : nullptr; p.n_rotations = n_rotations;
    p.rot_scale = mode == MODE_WHOLE ? 1 : 4;
    p.result_reg = rnd(VM_MAX_REGS);
    p.omega = with_omega ? omega : nullptr;
  }
  // made-up device addresses: the blob, the columns 2^40 bytes apart (no extent comes near that), the outputs
  const uint64_t dev = 0x100000000000ull + 256 * (uint64_t)rnd(1000), col0 = 0x700000000000ull, col_step = (uint64_t)1 << 40, out0 = 0x300000000000ull;
  std::vector<const void*> columns(n_columns);
  for (uint32_t i = 0; i < n_columns; i++) columns[i] = (const void*)(col0 + i * col_step);
  std::vector<uint32_t*> outs(n_progs);
  for (uint32_t j = 0; j < n_progs; j++) outs[j] = (uint32_t*)(out0 + j * col_step);
  const bool out_array = (ii + (int)n_progs) % 2 == 0;                 // the outputs as an array, or as a first address and a step
  const size_t out_step = 4;

  // ---- the plan
  const vm_blob_plan P = vm_blob_make_plan(progs.data(), n_progs, n_columns, log_rows);
  CHECK(P.regions.size() == n_progs);
  CHECK(row_vm_workspace_bytes(progs.data(), n_progs, n_columns, log_rows) == P.total);
  std::vector<std::pair<size_t, size_t>> pieces;                         // [start, end): the bytes somebody reads or writes
  auto piece = [&](size_t at, size_t bytes) { pieces.push_back({at, at + bytes}); return at % 256 == 0; };
  CHECK(piece(P.o_cols, (size_t)n_columns * 8));
  CHECK(piece(P.o_omega, 32));
  CHECK(piece(P.o_parts, (size_t)n_progs * sizeof(vm_part)));
  for (uint32_t j = 0; j < n_progs; j++) {
    const vm_blob_plan::region& r = P.regions[j];
    CHECK(piece(r.at, ((size_t)progs[j].n_insns + 4) * sizeof(vm_uop)));
    CHECK(piece(r.at + r.o_const, (size_t)progs[j].n_constants * 32 + 32));       // (the dummy operand reads 32 bytes even of an empty table)
    CHECK(piece(r.at + r.o_rot, (size_t)progs[j].n_rotations * 4 + 4));           // (the kernel's table lookup of slot 0)
  }
  const size_t staged_end = std::max_element(pieces.begin(), pieces.end(), [](auto& a, auto& b) { return a.second < b.second; })->second;
  CHECK(staged_end <= P.staged && P.staged == P.o_lo && P.staged % 256 == 0);
  CHECK(piece(P.o_lo, ((size_t)1 << POW_LO_BITS) * 32));
  CHECK(piece(P.o_hi, (size_t)std::max<uint64_t>(domain >> POW_LO_BITS, 1) * 32));
  CHECK(P.total % 256 == 0);
  std::sort(pieces.begin(), pieces.end());
  for (size_t i = 0; i + 1 < pieces.size(); i++) CHECK(pieces[i].second <= pieces[i + 1].first);
  CHECK(pieces.back().second <= P.total);

  // ---- the fill, into exactly `staged` bytes
  unsigned char* blob = (unsigned char*)calloc(P.staged, 1);
  if (!blob) return 2;
  vm_blob_fill(P, progs.data(), n_progs, columns.data(), n_columns, log_rows, window, with_omega ? omega : nullptr, out_array ? outs.data() : nullptr, outs[0],
               out_step, dev, blob);
  for (uint32_t i = 0; i < n_columns; i++) CHECK(std::memcmp(blob + P.o_cols + (size_t)i * 8, &columns[i], 8) == 0);
  if (with_omega) CHECK(std::memcmp(blob + P.o_omega, omega, 32) == 0);
  for (uint32_t j = 0; j < n_progs; j++) {
    const zkhip_vm_program& p = progs[j];
    const vm_blob_plan::region& r = P.regions[j];
    vm_part part;
    std::memcpy(&part, blob + P.o_parts + (size_t)j * sizeof(vm_part), sizeof part);
    const uint64_t d_region = dev + r.at, d_consts = d_region + r.o_const, consts_end = d_consts + vm_align256((size_t)p.n_constants * 32 + 32);
    CHECK((uint64_t)part.prog == d_region && (uint64_t)part.consts == d_consts && (uint64_t)part.rot_off == d_region + r.o_rot);
    CHECK(part.out == (out_array ? outs[j] : outs[0] + (size_t)j * out_step));
    CHECK(part.n_insns == p.n_insns && part.result_reg == p.result_reg);
    if (p.n_constants) CHECK(std::memcmp(blob + r.at + r.o_const, p.constants, (size_t)p.n_constants * 32) == 0);
    uint64_t halo_lo = 0, halo_hi = 0;
    if (window) row_vm_halos(&p, &halo_lo, &halo_hi);
    const uint64_t extent = window ? halo_lo + count + halo_hi : domain;         // elements of a column
    std::vector<int64_t> want_off(p.n_rotations);                                // the element a rotation reads at row 0
    for (uint32_t k = 0; k < p.n_rotations; k++) {
      const int64_t o = (int64_t)p.rotations[k] * p.rot_scale;
      want_off[k] = window ? (int64_t)halo_lo + o : ((o % (int64_t)domain) + (int64_t)domain) % (int64_t)domain;
      uint32_t got;
      std::memcpy(&got, blob + r.at + r.o_rot + (size_t)k * 4, 4);
      CHECK((int64_t)got == want_off[k] && (uint64_t)want_off[k] < extent);
    }
    for (uint32_t pc = 0; pc < p.n_insns + 4; pc++) {
      vm_uop u;
      std::memcpy(&u, blob + r.at + (size_t)pc * sizeof(vm_uop), sizeof u);
      zkhip_vm_insn got;
      std::memcpy(&got, &u, 16);
      zkhip_vm_insn want;
      if (pc >= p.n_insns) {                                                      // a padding no-op: MOV r0 <- r0
        std::memset(&want, 0, sizeof want);
        want.op = ZKHIP_OP_MOV; want.a.kind = ZKHIP_SRC_REG;
      } else {
        want = p.insns[pc];
        if ((want.op == ZKHIP_OP_MUL || want.op == ZKHIP_OP_MAD) && is_mem(want.a) != is_mem(want.b)) {
          if (is_mem(want.a)) std::swap(want.a, want.b);
          CHECK(is_mem(got.b) && !is_mem(got.a));                                 // exactly one memory operand: second
        }
      }
      CHECK(std::memcmp(&got, &want, 16) == 0);
      const bool uses_b = got.op == ZKHIP_OP_MUL || got.op == ZKHIP_OP_MAD || got.op == ZKHIP_OP_ADD || got.op == ZKHIP_OP_SUB;
      const zkhip_vm_operand* opnd[2] = {&got.a, &got.b};
      const uint64_t base[2] = {u.base_a, u.base_b};
      const uint32_t off[2] = {u.off_a, u.off_b}, mask[2] = {u.mask_a, u.mask_b};
      for (int k = 0; k < 2; k++) {
        const bool used = pc < p.n_insns && (k == 0 || uses_b);
        for (const uint64_t row : {(uint64_t)0, rows - 1}) {
          const uint64_t address = base[k] + (((row + off[k]) & wrap & (uint64_t)(int64_t)(int32_t)mask[k]) * 32);      // the kernel's rule
          if (mask[k]) {
            CHECK(mask[k] == 0xffffffffu && used && opnd[k]->kind == ZKHIP_SRC_COLUMN);
            const uint64_t column = (uint64_t)columns[opnd[k]->index];
            const uint64_t element = window ? row + (uint64_t)want_off[opnd[k]->rot] : (row + (uint64_t)want_off[opnd[k]->rot]) % domain;
            CHECK(address == column + element * 32 && element < extent);
          } else {
            CHECK(!(used && opnd[k]->kind == ZKHIP_SRC_COLUMN));
            CHECK(address >= d_consts && address + 32 <= consts_end);
            if (used && opnd[k]->kind == ZKHIP_SRC_CONST) CHECK(address == d_consts + (uint64_t)opnd[k]->index * 32);
          }
        }
      }
    }
  }
  free(blob);
  printf("%u %u %u %u %u %u %d %zu %zu\n", INSNS[ii], CONSTS[ci], ROTS[ri], n_columns, n_progs, log_rows, mode, P.staged, P.total);
  return 0;
}

int main() {
  int cases = 0;
  for (int ii = 0; ii < 6; ii++)
    for (int ci = 0; ci < 5; ci++)
      for (int ri = 0; ri < 4; ri++)
        for (uint32_t n_columns : COLUMNS)
          for (uint32_t n_progs : PROGS)
            for (uint32_t log_rows : LOG_ROWS)
              for (int mode = 0; mode < MODES; mode++) {
                if (n_progs == 257 && mode != (ii + ci + ri + (int)log_rows) % MODES) continue;      // (the long launches: one form per shape, in turn)
                const int rc = check_one(ii, ci, ri, n_columns, n_progs, log_rows, mode);
                if (rc) return rc;
                cases++;
              }
  printf("rowvm blob host check done: %d cases\n", cases);
  return 0;
}

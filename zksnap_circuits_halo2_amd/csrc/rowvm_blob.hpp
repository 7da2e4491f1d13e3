// What a launch of the row-program interpreter (rowvm.hip) reads from device memory besides the columns, as ONE blob the host fills and copies:
//   [column pointers | omega | part records | region of program 0 | region of program 1 | ... ]  [omega^j, j < 2^12 | omega^(j << 12)]
//    `staged` bytes: written by vm_blob_fill, one hipMemcpyAsync                                  the power tables: written by k_vm_pow_table
// with a region = [micro-ops (+ 4 padding no-ops) | constants | rotation offsets].  Every piece starts at a multiple of 256 bytes.  The
// layout is the same for every form -- one program, a window, several programs side by side (sums, checks) --: vm_blob_make_plan is the only
// place an offset is computed and `total` the workspace a call needs.  Host arithmetic that g++ compiles too, so that the plan and the fill
// can be executed on their own under a sanitizer (tests/cpp/rowvm_blob_host_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../include/zkhip.h"

namespace zkhip {

constexpr int VM_MAX_REGS = ZKHIP_VM_REGS;   // kernel variants exist for 6 / 8 / 12 / 16 registers (occupancy 4 / 3 / 2 / 2 waves per SIMD)
constexpr uint32_t POW_LO_BITS = 12;   // omega^row = hi[row >> 12] * lo[row & 4095]

// One instruction as the kernel reads it: the 16-byte instruction of the ABI plus, for its operands a and b, everything the address of their
// words needs -- base (a column's pointer, a constant's address, or a dummy for operands that are not in memory), rotation offset in rows and
// a row mask (all ones for a column, zero otherwise).  Resolved on the host (vm_blob_fill), so a fetch is ONE scalar load of 64 bytes and the
// operand loads depend on nothing else; the loop fetches two instructions ahead and loads operands one instruction ahead.
struct vm_uop {
  uint32_t head, oa, ob, oc;
  uint64_t base_a, base_b;
  uint32_t off_a, off_b, mask_a, mask_b;
  uint32_t pad[4];
};
static_assert(sizeof(vm_uop) == 64, "micro-op layout");
// what differs between the programs of a multi-program launch (the column table, the power tables and the rows are shared)
struct vm_part {
  const void* prog;
  const uint32_t* consts;
  const uint32_t* rot_off;
  uint32_t* out;
  uint32_t n_insns, result_reg;
};
static_assert(sizeof(vm_part) == 40, "the kernel reads a part record as five 64-bit words");
static_assert(sizeof(zkhip_vm_insn) == 16, "instruction layout");

inline size_t vm_align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct vm_blob_plan {
  struct region { size_t at, o_const, o_rot; };   // `at` from the blob's start; the constants and the rotation offsets from `at`
  size_t o_cols, o_omega, o_parts;
  std::vector<region> regions;                    // one per program
  size_t staged;                                  // bytes the host fills and copies = where the power tables begin
  size_t o_lo, o_hi, total;
};

// reads n_insns, n_constants and n_rotations of every program, nothing else
inline vm_blob_plan vm_blob_make_plan(const zkhip_vm_program* progs, uint32_t n_progs, uint32_t n_columns, uint32_t log_rows) {
  vm_blob_plan P;
  P.o_cols = 0;
  P.o_omega = P.o_cols + vm_align256((size_t)n_columns * 8 + 8);
  P.o_parts = P.o_omega + 256;
  size_t off = P.o_parts + vm_align256((size_t)n_progs * sizeof(vm_part));
  P.regions.resize(n_progs);
  for (uint32_t i = 0; i < n_progs; i++) {
    vm_blob_plan::region& r = P.regions[i];
    r.at = off;
    r.o_const = vm_align256(((size_t)progs[i].n_insns + 4) * sizeof(vm_uop));
    r.o_rot = r.o_const + vm_align256((size_t)progs[i].n_constants * 32 + 32);
    off += r.o_rot + vm_align256((size_t)progs[i].n_rotations * 4 + 4);
  }
  P.staged = P.o_lo = off;
  P.o_hi = P.o_lo + vm_align256(((size_t)1 << POW_LO_BITS) * 32);
  P.total = P.o_hi + vm_align256(((((size_t)1 << log_rows) >> POW_LO_BITS) + 1) * 32);
  return P;
}

// bytes of device workspace a launch of these programs needs
inline size_t row_vm_workspace_bytes(const zkhip_vm_program* progs, uint32_t n_progs, uint32_t n_columns, uint32_t log_rows) {
  return vm_blob_make_plan(progs, n_progs, n_columns, log_rows).total;
}

// halos of a window launch: o = rotation * rot_scale, not reduced; lo = max(0, -o), hi = max(0, o) over the rotation table
inline void row_vm_halos(const zkhip_vm_program* p, uint64_t* lo, uint64_t* hi) {
  int64_t l = 0, h = 0;
  for (uint32_t i = 0; i < p->n_rotations; i++) {
    const int64_t o = (int64_t)p->rotations[i] * (int64_t)p->rot_scale;
    l = std::max(l, -o);
    h = std::max(h, o);
  }
  *lo = (uint64_t)l;
  *hi = (uint64_t)h;
}

// highest register a program names (the kernel variant is sized for it)
inline uint32_t vm_top_register(const zkhip_vm_program* p) {
  uint32_t top = p->result_reg;
  for (uint32_t pc = 0; pc < p->n_insns; pc++) {
    const zkhip_vm_insn& in = p->insns[pc];
    if (in.dst > top) top = in.dst;
    const zkhip_vm_operand* o[3] = {&in.a, &in.b, &in.c};
    for (int k = 0; k < 3; k++) if (o[k]->kind == ZKHIP_SRC_REG && o[k]->index < (uint32_t)VM_MAX_REGS && o[k]->index > top) top = o[k]->index;
  }
  return top;
}

// The first P.staged bytes of the blob that will live at device address `dev`, into `blob` (host, zeroed by the caller).  Program i writes
// d_outs[i], or -- d_outs null -- d_out + i * out_step words.  `omega`: what the power tables are built from, or null.
// Micro-ops: the instruction + its operands' resolved addresses; a product's second factor is fetched scaled by 2^5 -- free for a column /
// constant (the other unpacking shift), a repack for a register -- so the memory operand goes second where the caller did not put it there.
// window: the columns are window buffers and a rotation's offset is halo_lo + rotation * rot_scale, not reduced; otherwise it is reduced
// modulo the domain.
inline void vm_blob_fill(const vm_blob_plan& P, const zkhip_vm_program* progs, uint32_t n_progs, const void* const* d_columns, uint32_t n_columns, uint32_t log_rows,
                         bool window, const uint64_t* omega, uint32_t* const* d_outs, uint32_t* d_out, size_t out_step, uint64_t dev, unsigned char* blob) {
  const int64_t rows = (int64_t)1 << log_rows;
  for (uint32_t i = 0; i < n_columns; i++) std::memcpy(blob + P.o_cols + (size_t)i * 8, &d_columns[i], 8);
  if (omega) std::memcpy(blob + P.o_omega, omega, 32);
  vm_part* parts = (vm_part*)(blob + P.o_parts);
  for (uint32_t i = 0; i < n_progs; i++) {
    const zkhip_vm_program* p = &progs[i];
    const vm_blob_plan::region& r = P.regions[i];
    const uint64_t d_region = dev + r.at, d_consts = d_region + r.o_const;
    parts[i].prog = (const void*)d_region;
    parts[i].consts = (const uint32_t*)d_consts;
    parts[i].rot_off = (const uint32_t*)(d_region + r.o_rot);
    parts[i].out = d_outs ? d_outs[i] : d_out + (size_t)i * out_step;
    parts[i].n_insns = p->n_insns;
    parts[i].result_reg = p->result_reg;
    uint32_t* rot_rows = (uint32_t*)(blob + r.at + r.o_rot);      // (a MAD's column addend still goes through this table)
    uint64_t halo_lo = 0, halo_hi = 0;
    if (window) row_vm_halos(p, &halo_lo, &halo_hi);
    for (uint32_t k = 0; k < p->n_rotations; k++) {
      const int64_t o = (int64_t)p->rotations[k] * (int64_t)p->rot_scale;
      rot_rows[k] = (uint32_t)(window ? (int64_t)halo_lo + o : ((o % rows) + rows) % rows);
    }
    if (p->n_constants) std::memcpy(blob + r.at + r.o_const, p->constants, (size_t)p->n_constants * 32);
    vm_uop* uops = (vm_uop*)(blob + r.at);
    for (uint32_t pc = 0; pc < p->n_insns + 4; pc++) {
      vm_uop& u = uops[pc];
      u.base_a = u.base_b = d_consts;                      // dummy address for operands that are not in memory (and for the padding no-ops)
      if (pc >= p->n_insns) { u.head = ZKHIP_OP_MOV | ((uint32_t)0 << 8); u.oa = ZKHIP_SRC_REG; continue; }   // MOV r0 <- r0 (never executed)
      zkhip_vm_insn in = p->insns[pc];
      const bool a_mem = in.a.kind == ZKHIP_SRC_COLUMN || in.a.kind == ZKHIP_SRC_CONST;
      const bool b_mem = in.b.kind == ZKHIP_SRC_COLUMN || in.b.kind == ZKHIP_SRC_CONST;
      if ((in.op == ZKHIP_OP_MUL || in.op == ZKHIP_OP_MAD) && a_mem && !b_mem) { const zkhip_vm_operand t = in.a; in.a = in.b; in.b = t; }
      std::memcpy(&u, &in, 16);
      const bool uses_b = in.op == ZKHIP_OP_MUL || in.op == ZKHIP_OP_MAD || in.op == ZKHIP_OP_ADD || in.op == ZKHIP_OP_SUB;
      auto resolve = [&](const zkhip_vm_operand& o, bool used, uint64_t* base, uint32_t* off, uint32_t* mask) {
        if (!used) return;
        if (o.kind == ZKHIP_SRC_COLUMN) { *base = (uint64_t)d_columns[o.index]; *off = rot_rows[o.rot]; *mask = 0xffffffffu; }
        else if (o.kind == ZKHIP_SRC_CONST) { *base = d_consts + (uint64_t)o.index * 32; }
      };
      resolve(in.a, true, &u.base_a, &u.off_a, &u.mask_a);
      resolve(in.b, uses_b, &u.base_b, &u.off_b, &u.mask_b);
    }
  }
}

}  // namespace zkhip

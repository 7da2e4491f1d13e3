// Drives the C++ mirror of the verifiers (include/zkhip.hpp: pairing_check, verify_opening, VerifierGWC, VerifierSHPLONK) on proofs that the
// mirror's own provers make; tests/test_gpu_verify.py::test_cpp_verifier_mirror reads the flags.
//   usage: verify_driver <k> <trapdoor> <g2.bin> <report.bin>      g2.bin: g2 | s_g2 as G2Affine memory (2 x 128 bytes; the mirror's setup makes no G2 points)
//   report: u64 flags, bit i set when expectation i holds:
//     0 verify_opening accepts   1 rejects value + 1          2 VerifierGWC accepts       3 rejects a changed evaluation
//     4 VerifierSHPLONK accepts  5 rejects a changed evaluation  6 rejects H and H' swapped  7 pairing_check of no pairs is true
//     8 both reject a changed evaluation on the REPETITION of a query (the plan's last query repeats (polynomial 2, x2): the set construction keeps
//       the first evaluation of a (polynomial, point) pair)   9 VerifierSHPLONK accepts one more agreeing repetition that the prover never saw
//     10 both reject one query of a polynomial opened several times carrying another polynomial's commitment
//   Polynomial 3 equals polynomial 0 (equal commitments, different point sets): every query carries a poly_id.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "zkhip.hpp"

using namespace zkhip::halo2;

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const uint32_t k = (uint32_t)std::atoi(argv[1]);
  const uint64_t trapdoor = std::strtoull(argv[2], nullptr, 0);
  const size_t n = (size_t)1 << k;
  try {
    init({0});
    ParamsKZG params = ParamsKZG::setup(k, detail::from_u64(trapdoor));
    {
      ParamsKZG::G2Bytes g2{}, s_g2{};
      FILE* in = fopen(argv[3], "rb");
      if (!in || fread(g2.data(), 128, 1, in) != 1 || fread(s_g2.data(), 128, 1, in) != 1) return 2;
      fclose(in);
      params.set_g2(g2, s_g2);
    }
    DeviceCommitter committer(params.get_g());
    std::array<uint8_t, 32> seed{};
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(i + k);
    std::vector<std::vector<Fr>> polys;
    for (uint64_t p = 0; p < 4; p++) polys.push_back(random_fr(seed, n, 0, p % 3));
    uint64_t flags = 0;
    const Fr x = detail::from_u64(0x1234567), x2 = detail::from_u64(0x89ABCDE), x3 = detail::from_u64(0x2468ACE);
    {   // one opening
      const Fr value = eval_polynomial(polys[0], x);
      std::vector<Fr> shifted = polys[0];
      shifted[0] = detail::sub_fr(shifted[0], value);
      std::vector<Fr> quot = kate_division(shifted, x);
      quot.push_back(Fr{});
      const G1 C = params.commit(polys[0]), W = params.commit(quot);
      if (verify_opening(params, C, x, value, W)) flags |= 1;
      if (!verify_opening(params, C, x, detail::add_fr(value, detail::one()), W)) flags |= 2;
    }
    std::vector<DeviceVec> d_polys;
    for (const auto& p : polys) d_polys.emplace_back(p);
    std::vector<G1> commitments;
    for (const auto& d : d_polys) commitments.push_back(committer.commit(d.data()));
    const uint32_t which[] = {0, 1, 1, 2, 2, 2, 3, 0, 2};
    const Fr* pts[] = {&x, &x, &x2, &x, &x2, &x3, &x3, &x3, &x2};
    std::vector<ProverQuery> queries;
    std::vector<VerifierQuery> vq;
    for (int i = 0; i < 9; i++) {
      queries.push_back(ProverQuery{*pts[i], &d_polys[which[i]]});
      vq.push_back(VerifierQuery{*pts[i], commitments[which[i]], eval_polynomial(polys[which[i]], *pts[i]), &d_polys[which[i]]});
    }
    const Fr y = detail::from_u64(77777), v = detail::from_u64(88888), u = detail::from_u64(99999);
    const std::vector<G1> W = gwc_create_proof(committer, k, queries, v);
    const std::pair<G1, G1> HH = shplonk_create_proof(committer, k, queries, y, v, u);
    std::vector<VerifierQuery> bad = vq;
    bad[4].eval = detail::add_fr(bad[4].eval, detail::one());
    if (VerifierGWC(params).verify_proof(vq, W, v, u)) flags |= 4;
    if (!VerifierGWC(params).verify_proof(bad, W, v, u)) flags |= 8;
    if (VerifierSHPLONK(params).verify_proof(vq, HH.first, HH.second, y, v, u)) flags |= 16;
    if (!VerifierSHPLONK(params).verify_proof(bad, HH.first, HH.second, y, v, u)) flags |= 32;
    if (!VerifierSHPLONK(params).verify_proof(vq, HH.second, HH.first, y, v, u)) flags |= 64;
    if (pairing_check({}, {})) flags |= 128;
    {
      std::vector<VerifierQuery> rep = vq;
      rep[8].eval = detail::add_fr(rep[8].eval, detail::one());
      if (!VerifierGWC(params).verify_proof(rep, W, v, u) && !VerifierSHPLONK(params).verify_proof(rep, HH.first, HH.second, y, v, u)) flags |= 256;
      rep = vq;
      rep.push_back(vq[0]);
      if (VerifierSHPLONK(params).verify_proof(rep, HH.first, HH.second, y, v, u)) flags |= 512;
      std::vector<VerifierQuery> swapped = vq;
      swapped[4].commitment = commitments[1];                 // polynomial 2 is opened at three points: one of its queries names polynomial 1's commitment
      if (!VerifierGWC(params).verify_proof(swapped, W, v, u) && !VerifierSHPLONK(params).verify_proof(swapped, HH.first, HH.second, y, v, u)) flags |= 1024;
    }
    FILE* rep = fopen(argv[4], "wb");
    if (!rep) return 2;
    fwrite(&flags, 8, 1, rep);
    fclose(rep);
  } catch (const std::exception& e) {
    fprintf(stderr, "verify_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}

/* C99 through include/zkhip.h alone: the transcript's host calls in a process that never touches a GPU.  A fresh writer's first squeeze is the
 * header's pin; a scalar written and read back gives the same second challenge on both sides.  Prints the first challenge's 4 Montgomery
 * words (tests/test_transcript_host.py decodes them) and "transcript driver OK". */
#include <stdio.h>
#include <string.h>
#include "zkhip.h"

/* 0x0e89c2c9ef365f095ec7aa36500bb0ba58bf7d5e17194055afb5a1c746f1786a times 2^256 mod r */
static const uint64_t PIN_MONT[4] = {0x3c49925d7da9a625ULL, 0x0b56f8ac0a0dec42ULL, 0x1a8d03ed3c823c30ULL, 0x0faad4aeeabf601aULL};

int main(void) {
  uint64_t c0[4], c1[4], r0[4], r1[4], back[4];
  uint8_t proof[64];
  size_t len = 0;
  zkhip_transcript *w = zkhip_transcript_new(0), *r;
  if (!w) return 1;
  if (zkhip_transcript_squeeze(w, c0) != ZKHIP_OK) return 2;
  printf("%016llx %016llx %016llx %016llx\n", (unsigned long long)c0[0], (unsigned long long)c0[1], (unsigned long long)c0[2], (unsigned long long)c0[3]);
  if (memcmp(c0, PIN_MONT, 32) != 0) return 3;
  if (zkhip_transcript_write_scalars(w, c0, 1) != ZKHIP_OK) return 4;
  if (zkhip_transcript_squeeze(w, c1) != ZKHIP_OK) return 5;
  if (zkhip_transcript_proof(w, NULL, 0, &len) != ZKHIP_OK || len != 32) return 6;
  if (zkhip_transcript_proof(w, proof, sizeof(proof), &len) != ZKHIP_OK) return 7;
  if (zkhip_transcript_read_scalars(w, 1, back) != ZKHIP_EINVAL) return 8;     /* a writer does not read */
  r = zkhip_transcript_new_reader(proof, len, 0);
  if (!r) return 9;
  if (zkhip_transcript_squeeze(r, r0) != ZKHIP_OK || memcmp(r0, c0, 32) != 0) return 10;
  if (zkhip_transcript_read_scalars(r, 1, back) != ZKHIP_OK || memcmp(back, c0, 32) != 0) return 11;
  if (zkhip_transcript_squeeze(r, r1) != ZKHIP_OK || memcmp(r1, c1, 32) != 0) return 12;
  if (zkhip_transcript_read_scalars(r, 1, back) != ZKHIP_EINVAL) return 13;    /* past the end */
  zkhip_transcript_free(r);
  zkhip_transcript_free(w);
  printf("transcript driver OK\n");
  return 0;
}

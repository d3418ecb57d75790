// rlc_weights.h -- the secret weights of nbls_verify_multiple (random-linear-combination batch verification of independent signatures):
//   r_i = BE64(SHA-256(seed32 || BE64(i))[0..8]) | 2^63, stored as a 32-byte big-endian scalar with 24 leading zero bytes,
// so that the G2 MSM reads it with nbits = 64 and the 64-bit G1 ladder (P_G1_MUL64) reads its low 8 bytes.  The top bit makes every weight non-zero and of one length
// (the ladder's one-bit top window).  Written once and compiled twice like scalar_split.h: into msm_kernels.hip (one thread per set) and into the test-only simulator
// (tests/test_verify_multiple_sim.py checks it against hashlib).  The 40-byte message is ONE block: seed, index, 0x80, zeros, the bit length 320.
#pragma once
#include <stdint.h>
#include "sha256.h"

namespace nbls {

NBLS_SHA_HD void rlc_weight(const uint8_t* seed32, uint64_t i, uint8_t* out32) {
  uint32_t w[16], h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  for (int k = 0; k < 8; k++) w[k] = ((uint32_t)seed32[4 * k] << 24) | ((uint32_t)seed32[4 * k + 1] << 16) | ((uint32_t)seed32[4 * k + 2] << 8) | seed32[4 * k + 3];
  w[8] = (uint32_t)(i >> 32); w[9] = (uint32_t)i; w[10] = 0x80000000u;
  for (int k = 11; k < 15; k++) w[k] = 0;
  w[15] = 40 * 8;
  sha256_compress(h, w);
  for (int k = 0; k < 24; k++) out32[k] = 0;
  const uint32_t hi = h[0] | 0x80000000u, lo = h[1];
  for (int k = 0; k < 4; k++) { out32[24 + k] = (uint8_t)(hi >> (24 - 8 * k)); out32[28 + k] = (uint8_t)(lo >> (24 - 8 * k)); }
}

}  // namespace nbls

// csrc/composite.hip: the keep window that borrows the halo buffer, and the two-buffer hand-off between the blur passes
// (halo -> horizontal pass -> vertical pass, three channels in turn).  argv[1]: r_lo (default 32; 64 = widest halo)
#include EMU_SOURCE
#include "common.h"
int main(int argc, char** argv) {
  const int r_lo = argc > 1 ? atoi(argv[1]) : 32;
  const int B = 2, th = 4, tw = 3, cell = 16, H = th * cell, W = tw * cell;  // 64 x 48: 2 x 2 tiles, the right ones ragged
  const double sigma = r_lo / 4.0;
  const int R = std::min(32, (int)ceil(3.0 * sigma));
  std::vector<float> taps(2 * R + 1);
  double sum = 0.0;
  for (int k = -R; k <= R; ++k) sum += exp(-0.5 * (k / sigma) * (k / sigma));
  for (int k = -R; k <= R; ++k) taps[k + R] = (float)(exp(-0.5 * (k / sigma) * (k / sigma)) / sum);
  std::vector<float> dec((size_t)B * 3 * H * W), photo(dec.size()), out(dec.size());
  std::vector<uint8_t> keep(B * th * tw, 1), u8((size_t)B * H * W * 3);
  fill(dec, 0.25f); fill(photo, 0.5f);
  keep[1 * tw + 1] = 0;  // image 0: one interior cell (every tile blends); image 1: nothing edited (every tile copies)
  int rc = t2h_composite_region_f32(dec.data(), photo.data(), keep.data(), taps.data(), out.data(), u8.data(), B, H, W, th,
                                    tw, 4, r_lo, R, 1, nullptr);
  printf("rc %d\n", rc);
  return rc;
}

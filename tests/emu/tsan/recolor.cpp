// csrc/recolor.hip: the membership codes staged in LDS with their classification word, and the hand-off between the
// two integer passes of the tent filter (codes -> horizontal pass -> vertical pass); the statistics' LDS hand-over of
// the wave sums runs first.  argv[1]: feather (default 2; 8 = widest halo)
#include EMU_SOURCE
#include "common.h"
int main(int argc, char** argv) {
  const int f = argc > 1 ? atoi(argv[1]) : 2;
  const int B = 2, G = 2, H = 64, W = 44;  // 2 x 2 tiles, the right ones ragged
  std::vector<float> img((size_t)B * 3 * H * W), out(img.size()), segm((size_t)B * H * W, 0.f);
  std::vector<uint8_t> u8((size_t)B * H * W * 3);
  fill(img, 0.25f);
  // image 0: two touching regions across the tile seams (every tile filters); image 1: one group everywhere
  for (int y = 20; y < 50; ++y)
    for (int x = 10; x < 40; ++x) segm[(size_t)y * W + x] = x < 30 ? 1.f : 3.f;
  for (size_t i = 0; i < (size_t)H * W; ++i) segm[(size_t)H * W + i] = 4.f;
  const uint64_t bits[2] = {(1ull << 1) | (1ull << 4), (1ull << 3) | (1ull << 5) | (1ull << 21)};
  std::vector<double> partial((size_t)B * ((H + 15) / 16) * G * 8), src((size_t)B * G * 8), dst;
  int rc = t2h_region_color_stats(img.data(), 0, segm.data(), bits, G, B, H, W, partial.data(), src.data(), nullptr);
  dst = src;
  for (int i = 0; i < B * G; ++i)
    if (src[i * 8] > 0) dst[i * 8 + 2] += 0.1;
  if (rc == 0)
    rc = t2h_recolor_region_f32(img.data(), 0, segm.data(), bits, G, src.data(), dst.data(), 1.f, 4.f, f, out.data(),
                                u8.data(), B, H, W, nullptr);
  printf("rc %d\n", rc);
  return rc;
}

// csrc/vq_fit.hip: the all-codebook fit (double-buffered operand tiles, code norms and the final wave merge through LDS)
// on the row tile given as the argument (32 / 64 / 128), then the region vote
#include EMU_SOURCE
#include "common.h"
int main(int argc, char** argv) {
  const int tile = argc > 1 ? atoi(argv[1]) : 0;
  const int n = 40, nb = 1, n_e = 130, d = 256;  // two row tiles of 32, a row-tile tail, a code-tile tail
  std::vector<float> z(n * d), books((size_t)nb * n_e * d), dmin(n * nb);
  std::vector<int32_t> jmin(n * nb);
  fill(z); fill(books);
  t2h_vq_fit_force_tile(tile);
  int rc = t2h_vq_fit_books_f32(z.data(), books.data(), dmin.data(), jmin.data(), n, nb, n_e, d, nullptr);
  const int B = 2, T = n / B;
  std::vector<int64_t> segm(n), attr(B * 3);
  for (int i = 0; i < n; ++i) segm[i] = i % 6;
  std::vector<double> cost(B * 3 * nb);
  std::vector<int32_t> count(B * 3);
  rc |= t2h_texture_vote(dmin.data(), segm.data(), B, T, nb, cost.data(), count.data(), attr.data(), nullptr);
  printf("rc %d\n", rc);
  return rc;
}

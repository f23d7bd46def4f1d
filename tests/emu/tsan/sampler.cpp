// csrc/sampler.hip: the row-threshold selection of truncated sampling (LDS histograms filled by atomics, read and zeroed
// by plain accesses of the first wave, the selected bin handed back through LDS) at the workgroup and the wave scope
#include EMU_SOURCE
#include "common.h"
int main(int, char**) {
  const int n_rows = 6, n_class = 1024;
  std::vector<float> logits((size_t)n_rows * n_class), theta(n_rows);
  std::vector<int32_t> kept(n_rows);
  fill(logits, 2.f);
  for (int j = 0; j < n_class; ++j) logits[j] = (float)(j % 7);  // a row of ties
  int rc = 0;
  for (int scope = 0; scope < 2; ++scope) {
    rc |= t2h_truncation_threshold(logits.data(), n_rows, n_class, 64, 0, scope, theta.data(), kept.data(), nullptr);
    rc |= t2h_truncation_threshold(logits.data(), n_rows, n_class, 0, 943718, scope, theta.data(), kept.data(), nullptr);
    rc |= t2h_truncation_threshold(logits.data(), n_rows, n_class, 300, 524288, scope, theta.data(), kept.data(), nullptr);
  }
  printf("rc %d\n", rc);
  return rc;
}

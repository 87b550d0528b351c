// The host-side argument checks of the mean-scale entry points (csrc/meancodec.hip), as a stand-alone program
// for a sanitized CPU build: `make -C image_compression_amd/csrc hostcheck` compiles meancodec.hip's host code
// and this file with -fsanitize=address,undefined and runs the result.  Every call below must be refused with
// IC_ERR_ARG before anything touches a device, so the program needs no GPU; the pointers are real host
// allocations (never dereferenced by a correct check, and the sanitizers watch them if one is).
#include <cstdio>
#include <limits>
#include <vector>

#include "../include/imgcomp.h"

static int failures = 0;

#define EXPECT_ARG(call)                                              \
  do {                                                                \
    const int rc_ = (call);                                           \
    if (rc_ != IC_ERR_ARG) {                                          \
      std::printf("FAIL %s -> %d (line %d)\n", #call, rc_, __LINE__); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

int main() {
  std::vector<float> y(8, 1.f), mu(8, 0.25f), r(8), y_hat(8);
  std::vector<int> sym(8), kdev(3), khost(3, -1);
  const long long big = std::numeric_limits<long long>::max();
  float* const nf = nullptr;
  int* const ni = nullptr;

  // null operands, one at a time
  EXPECT_ARG(ic_codec_symbolize_mean(nf, mu.data(), 8, sym.data(), kdev.data(), khost.data(), nullptr));
  EXPECT_ARG(ic_codec_symbolize_mean(y.data(), nf, 8, sym.data(), kdev.data(), khost.data(), nullptr));
  EXPECT_ARG(ic_codec_symbolize_mean(y.data(), mu.data(), 8, ni, kdev.data(), khost.data(), nullptr));
  EXPECT_ARG(ic_codec_symbolize_mean(y.data(), mu.data(), 8, sym.data(), ni, khost.data(), nullptr));
  EXPECT_ARG(ic_codec_symbolize_mean(y.data(), mu.data(), 8, sym.data(), kdev.data(), ni, nullptr));
  EXPECT_ARG(ic_codec_symbolize_mean_seg(nf, mu.data(), 2, 4, sym.data(), kdev.data(), khost.data(), nullptr));
  EXPECT_ARG(ic_codec_symbolize_mean_seg(y.data(), nf, 2, 4, sym.data(), kdev.data(), khost.data(), nullptr));
  EXPECT_ARG(ic_codec_symbolize_mean_seg(y.data(), mu.data(), 2, 4, ni, kdev.data(), khost.data(), nullptr));
  EXPECT_ARG(ic_codec_symbolize_mean_seg(y.data(), mu.data(), 2, 4, sym.data(), ni, khost.data(), nullptr));
  EXPECT_ARG(ic_codec_symbolize_mean_seg(y.data(), mu.data(), 2, 4, sym.data(), kdev.data(), ni, nullptr));
  EXPECT_ARG(ic_center_round(nf, mu.data(), 8, r.data(), y_hat.data(), nullptr));
  EXPECT_ARG(ic_center_round(y.data(), nf, 8, r.data(), y_hat.data(), nullptr));
  EXPECT_ARG(ic_center_round(y.data(), mu.data(), 8, nf, y_hat.data(), nullptr));
  EXPECT_ARG(ic_center_round(y.data(), mu.data(), 8, r.data(), nf, nullptr));
  EXPECT_ARG(ic_add_mean(nf, mu.data(), 8, y_hat.data(), nullptr));
  EXPECT_ARG(ic_add_mean(r.data(), nf, 8, y_hat.data(), nullptr));
  EXPECT_ARG(ic_add_mean(r.data(), mu.data(), 8, nf, nullptr));

  // zero and negative lengths
  for (long long n : {0ll, -1ll, std::numeric_limits<long long>::min()}) {
    EXPECT_ARG(ic_codec_symbolize_mean(y.data(), mu.data(), n, sym.data(), kdev.data(), khost.data(), nullptr));
    EXPECT_ARG(ic_codec_symbolize_mean_seg(y.data(), mu.data(), 2, n, sym.data(), kdev.data(), khost.data(), nullptr));
    EXPECT_ARG(ic_center_round(y.data(), mu.data(), n, r.data(), y_hat.data(), nullptr));
    EXPECT_ARG(ic_add_mean(r.data(), mu.data(), n, y_hat.data(), nullptr));
  }

  // mismatched arguments: segment counts and lengths that do not describe one buffer (no segments, more than
  // a launch's 65535, a product past 2^63), and the quantiser's two outputs in one place
  for (int nseg : {0, -3, 65536, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()})
    EXPECT_ARG(ic_codec_symbolize_mean_seg(y.data(), mu.data(), nseg, 4, sym.data(), kdev.data(), khost.data(), nullptr));
  EXPECT_ARG(ic_codec_symbolize_mean_seg(y.data(), mu.data(), 3, big / 2, sym.data(), kdev.data(), khost.data(), nullptr));
  EXPECT_ARG(ic_codec_symbolize_mean_seg(y.data(), mu.data(), 65535, big / 65535 + 1, sym.data(), kdev.data(), khost.data(),
                                         nullptr));
  EXPECT_ARG(ic_center_round(y.data(), mu.data(), 8, r.data(), r.data(), nullptr));

  for (int k : khost)
    if (k != -1) {
      std::printf("FAIL a refused call wrote kmax_host\n");
      ++failures;
    }
  std::printf(failures ? "meancodec host checks: %d FAILED\n" : "meancodec host checks: ok (%d failures)\n", failures);
  return failures ? 1 : 0;
}

// The host-side argument checks of the requantizer (csrc/transcode.hip), as a stand-alone program for a sanitized
// CPU build: `make -C image_compression_amd/csrc hostcheck` compiles transcode.hip's host code and this file with
// -fsanitize=address,undefined and runs the result.  Every call below must be refused with IC_ERR_ARG before anything
// touches a device, so the program needs no GPU; the pointers are real host allocations of exactly the sizes the
// arguments name, so a check that reads past the img array is caught by the sanitizers.
#include <cstdio>
#include <vector>

#include "../include/imgcomp.h"

static int failures = 0;

#define EXPECT_RC(want, call)                                                   \
  do {                                                                          \
    const int rc_ = (call);                                                     \
    if (rc_ != (want)) {                                                        \
      std::printf("FAIL %s -> %d, not %d (line %d)\n", #call, rc_, (want), __LINE__); \
      ++failures;                                                               \
    }                                                                           \
  } while (0)

namespace {

// A valid call: two sources of 7 positions of 5 channels, five targets.  One member is edited; the call must then be
// refused.
struct Call {
  long long N = 2, P = 7;
  int C = 5, nseg = 5;
  std::vector<float> r = std::vector<float>(2 * 7 * 5, 1.f), mu1 = r, a = std::vector<float>(2 * 5, 1.f),
                     b = std::vector<float>(5 * 5, 1.f), mu2 = std::vector<float>(5 * 7 * 5, 0.f);
  std::vector<int> img = {0, 1, 1, 0, 1}, img_dev = std::vector<int>(5, -1), sym = std::vector<int>(5 * 7 * 5, -1),
                   kmax_dev = std::vector<int>(5, -1), kmax_host = std::vector<int>(5, -1);
  const float *pr = r.data(), *pm1 = mu1.data(), *pa = a.data(), *pb = b.data(), *pm2 = mu2.data();
  const int* pimg = img.data();
  int *pdev = img_dev.data(), *psym = sym.data(), *pkd = kmax_dev.data(), *pkh = kmax_host.data();

  int run() { return ic_requant_seg(pr, pm1, N, P, C, pa, pb, pm2, nseg, pimg, pdev, psym, pkd, pkh, nullptr); }
};

template <class Edit>
void refused(int line, Edit edit) {
  Call c;
  edit(c);
  const int rc = c.run();
  if (rc != IC_ERR_ARG) {
    std::printf("FAIL the call edited at line %d -> %d, not %d\n", line, rc, IC_ERR_ARG);
    ++failures;
  }
  for (int v : c.sym)
    if (v != -1) {
      std::printf("FAIL the call edited at line %d wrote its output\n", line);
      ++failures;
      break;
    }
}

}  // namespace

int main() {
  // every null pointer
  refused(__LINE__, [](Call& c) { c.pr = nullptr; });
  refused(__LINE__, [](Call& c) { c.pm1 = nullptr; });
  refused(__LINE__, [](Call& c) { c.pa = nullptr; });
  refused(__LINE__, [](Call& c) { c.pb = nullptr; });
  refused(__LINE__, [](Call& c) { c.pm2 = nullptr; });
  refused(__LINE__, [](Call& c) { c.pimg = nullptr; });
  refused(__LINE__, [](Call& c) { c.pdev = nullptr; });
  refused(__LINE__, [](Call& c) { c.psym = nullptr; });
  refused(__LINE__, [](Call& c) { c.pkd = nullptr; });
  refused(__LINE__, [](Call& c) { c.pkh = nullptr; });
  // N and nseg in [1, 65535], P and C >= 1
  for (long long n : {0ll, -1ll, 65536ll}) refused(__LINE__, [n](Call& c) { c.N = n; });
  for (int n : {0, -2, 65536}) refused(__LINE__, [n](Call& c) { c.nseg = n; });
  for (long long p : {0ll, -7ll}) refused(__LINE__, [p](Call& c) { c.P = p; });
  for (int ch : {0, -5}) refused(__LINE__, [ch](Call& c) { c.C = ch; });
  // the extent overflow guard: P * C * max(N, nseg) beyond 2^63
  refused(__LINE__, [](Call& c) { c.P = 1ll << 62; });
  refused(__LINE__, [](Call& c) { c.P = 0x7fffffffffffffffll / 5 / 5 + 1; });
  // img outside [0, N), first and last entry
  refused(__LINE__, [](Call& c) { c.img[0] = 2; });
  refused(__LINE__, [](Call& c) { c.img[4] = -1; });
  refused(__LINE__, [](Call& c) { c.img[2] = 65535; });
  // one source only: every img entry but 0 is outside
  refused(__LINE__, [](Call& c) { c.N = 1; });

  std::printf(failures ? "transcode host checks: %d FAILED\n" : "transcode host checks: ok (%d failures)\n", failures);
  return failures ? 1 : 0;
}

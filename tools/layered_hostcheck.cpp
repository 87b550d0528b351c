// The host-side argument checks of the layered-stream kernels (csrc/layered.hip), as a stand-alone program for a
// sanitized CPU build: `make -C image_compression_amd/csrc hostcheck` compiles layered.hip's host code and this file
// with -fsanitize=address,undefined and runs the result.  Every call below must be refused with IC_ERR_ARG before
// anything touches a device, so the program needs no GPU; the pointers are real host allocations of exactly the
// sizes the arguments name, so a check that reads past an order, seg or nlayers array is caught by the sanitizers.
#include <cstdio>
#include <limits>
#include <vector>

#include "../include/imgcomp.h"

static int failures = 0;

namespace {

// A valid call of each entry point: N = 2 images, P = 6 positions, C = 8 channels in G = 4 layers of 2; image 0 in
// identity order, image 1 reversed.  `edit` changes one thing; the call must then be refused and write nothing.
struct Call {
  static constexpr int N0 = 2, C0 = 8, G0 = 4;
  static constexpr long long P0 = 6;
  int n = N0, c = C0, g = G0, elem = 4, nseg = 3;
  long long p = P0;
  std::vector<int> sym = std::vector<int>(N0 * P0 * C0, 1);
  std::vector<float> mu = std::vector<float>(N0 * P0 * C0, 0.5f);
  std::vector<int> order, seg = {1, 3, 0, 0, 1, 3}, nlayers = {4, 1};
  std::vector<int> order_dev = std::vector<int>(N0 * C0, -1);
  std::vector<int> seg_dev = std::vector<int>(4 * 3 + N0 + 1, -1), nl_dev = std::vector<int>(2 * N0, -1);
  std::vector<unsigned long long> energy = std::vector<unsigned long long>(N0 * C0, 7);
  std::vector<int> dst = std::vector<int>(3 * P0 * (C0 / G0), -1);
  std::vector<float> q = std::vector<float>(5 * P0 * (C0 / G0), 2.f), y_hat = std::vector<float>(N0 * P0 * C0, -1.f);
  bool null_sym = false, null_energy = false, null_src = false, null_order = false, null_order_dev = false,
       null_seg = false, null_seg_dev = false, null_dst = false, null_q = false, null_nl = false, null_nl_dev = false,
       null_y = false;

  Call() {
    for (int i = 0; i < C0; ++i) order.push_back(i);
    for (int i = 0; i < C0; ++i) order.push_back(C0 - 1 - i);
  }
  int run_energy() {
    return ic_layer_energy(null_sym ? nullptr : sym.data(), n, p, c, null_energy ? nullptr : energy.data(), nullptr);
  }
  int run_gather() {
    return ic_layer_gather(null_src ? nullptr : sym.data(), elem, n, p, c, g, null_order ? nullptr : order.data(),
                           null_order_dev ? nullptr : order_dev.data(), null_seg ? nullptr : seg.data(),
                           null_seg_dev ? nullptr : seg_dev.data(), nseg, null_dst ? nullptr : dst.data(), nullptr);
  }
  int run_scatter() {
    return ic_layer_scatter(null_q ? nullptr : q.data(), mu.data(), n, p, c, g, null_order ? nullptr : order.data(),
                            null_order_dev ? nullptr : order_dev.data(), null_nl ? nullptr : nlayers.data(),
                            null_nl_dev ? nullptr : nl_dev.data(), null_y ? nullptr : y_hat.data(), nullptr);
  }
  bool untouched() const {
    for (int v : order_dev)
      if (v != -1) return false;
    for (int v : seg_dev)
      if (v != -1) return false;
    for (int v : nl_dev)
      if (v != -1) return false;
    for (int v : dst)
      if (v != -1) return false;
    for (float v : y_hat)
      if (v != -1.f) return false;
    for (unsigned long long v : energy)
      if (v != 7) return false;
    return true;
  }
};

enum { ENERGY = 1, GATHER = 2, SCATTER = 4, ALL = 7 };

template <class Edit>
void refused(int line, int which, Edit edit) {
  for (int k : {ENERGY, GATHER, SCATTER}) {
    if (!(which & k)) continue;
    Call c;
    edit(c);
    const int rc = k == ENERGY ? c.run_energy() : k == GATHER ? c.run_gather() : c.run_scatter();
    if (rc != IC_ERR_ARG) {
      std::printf("FAIL the edit of line %d, entry point %d -> %d, not %d\n", line, k, rc, IC_ERR_ARG);
      ++failures;
    }
    if (!c.untouched()) {
      std::printf("FAIL the refused call of line %d, entry point %d wrote an output\n", line, k);
      ++failures;
    }
  }
}
#define REFUSED(which, ...) refused(__LINE__, which, [](Call& c) { __VA_ARGS__; })

}  // namespace

int main() {
  const int imax = std::numeric_limits<int>::max(), imin = std::numeric_limits<int>::min();
  const long long lmax = std::numeric_limits<long long>::max(), lmin = std::numeric_limits<long long>::min();

  // null operands, one at a time (mu may be NULL; q only when no layer is present)
  REFUSED(ENERGY, c.null_sym = true);
  REFUSED(ENERGY, c.null_energy = true);
  REFUSED(GATHER, c.null_src = true);
  REFUSED(GATHER | SCATTER, c.null_order = true);
  REFUSED(GATHER | SCATTER, c.null_order_dev = true);
  REFUSED(GATHER, c.null_seg = true);
  REFUSED(GATHER, c.null_seg_dev = true);
  REFUSED(GATHER, c.null_dst = true);
  REFUSED(SCATTER, c.null_q = true);
  REFUSED(SCATTER, c.null_nl = true);
  REFUSED(SCATTER, c.null_nl_dev = true);
  REFUSED(SCATTER, c.null_y = true);

  // N, P, C, G below 1; C % G != 0; G > C
  for (int v : {0, -1, imin}) {
    refused(__LINE__, ALL, [v](Call& c) { c.n = v; });
    refused(__LINE__, ALL, [v](Call& c) { c.c = v; });
    refused(__LINE__, GATHER | SCATTER, [v](Call& c) { c.g = v; });
  }
  for (long long v : {0ll, -1ll, lmin}) refused(__LINE__, ALL, [v](Call& c) { c.p = v; });
  for (int v : {3, 5, 7, 9, 16, imax}) refused(__LINE__, GATHER | SCATTER, [v](Call& c) { c.g = v; });

  // an extent beyond 2^63 (and beyond the 2^60 elements whose byte offsets stay below it)
  for (long long v : {lmax, lmax / 2, lmax / 16, (1ll << 60) / 16 + 1}) refused(__LINE__, ALL, [v](Call& c) { c.p = v; });

  // elem_bytes outside {1, 4}
  for (int v : {0, 2, 3, 8, -4, imax, imin}) refused(__LINE__, GATHER, [v](Call& c) { c.elem = v; });

  // nseg outside 1 .. 65535
  for (int v : {0, -1, 65536, imax, imin}) refused(__LINE__, GATHER, [v](Call& c) { c.nseg = v; });

  // a seg entry out of range: the image in [0, N), the layer in [0, G)
  for (int v : {-1, 2, imax, imin}) {
    refused(__LINE__, GATHER, [v](Call& c) { c.seg[0] = v; });
    refused(__LINE__, GATHER, [v](Call& c) { c.seg[4] = v; });
  }
  for (int v : {-1, 4, imax, imin}) {
    refused(__LINE__, GATHER, [v](Call& c) { c.seg[1] = v; });
    refused(__LINE__, GATHER, [v](Call& c) { c.seg[5] = v; });
  }

  // an nlayers entry out of range: 0 .. G
  for (int v : {-1, 5, imax, imin}) {
    refused(__LINE__, SCATTER, [v](Call& c) { c.nlayers[0] = v; });
    refused(__LINE__, SCATTER, [v](Call& c) { c.nlayers[1] = v; });
  }

  // an order row that is not a permutation: a repeat, a value out of range, in either row
  REFUSED(GATHER | SCATTER, c.order[3] = 2);
  REFUSED(GATHER | SCATTER, c.order[15] = 1);
  for (int v : {-1, 8, imax, imin}) {
    refused(__LINE__, GATHER | SCATTER, [v](Call& c) { c.order[0] = v; });
    refused(__LINE__, GATHER | SCATTER, [v](Call& c) { c.order[8] = v; });
  }

  // overlapping operands
  {
    Call c;
    if (ic_layer_gather(c.sym.data(), 4, c.n, c.p, c.c, c.g, c.order.data(), c.order_dev.data(), c.seg.data(),
                        c.seg_dev.data(), c.nseg, c.sym.data(), nullptr) != IC_ERR_ARG ||
        ic_layer_scatter(c.q.data(), c.mu.data(), c.n, c.p, c.c, c.g, c.order.data(), c.order_dev.data(),
                         c.nlayers.data(), c.nl_dev.data(), c.mu.data(), nullptr) != IC_ERR_ARG) {
      std::printf("FAIL an output that is an input was not refused\n");
      ++failures;
    }
  }

  std::printf(failures ? "layered host checks: %d FAILED\n" : "layered host checks: ok (%d failures)\n", failures);
  return failures ? 1 : 0;
}

// Coding to a byte budget: the symbols of y for M candidate (image, quality) pairs in one launch
// (ic_gain_symbolize_seg).  Candidate m names its image img[m] of the N-image latent y and its own gain row g[m];
// its mean mu[m] and its symbols sym[m] are segments of P * C elements back to back:
//     sym[m][i] = symbol_of(sub_rn(mul_rn(y[img[m]][i], g[m][c(i)]), mu[m][i]))
// The product is ic_channel_scale's one fp32 multiplication and the difference ic_codec_symbolize_mean_seg's one fp32
// subtraction (fp_rn.h: each rounded once, neither contracted with the other): bit for bit those two calls on the
// gathered batch y[img], without the gather copy and without the scaled latent in memory.
// y, mu and sym are dense channels-last storage (P positions, channel fastest).  The walk and the driver are
// seg_symbolize.h's: 16-byte accesses when every pointer is 16-byte aligned and C % 4 == 0 (then every segment and
// every gain row starts on a 16-byte boundary and a group of four never straddles a position).
#include <algorithm>

#include "seg_symbolize.h"

namespace {

struct GainSrc {
  const float *y, *g, *mu;
  const int* img;
  ChannelCursor ch;
  __device__ __forceinline__ void bind(unsigned seg, long long len, long long first, long long per) {
    y += (long long)img[seg] * len;
    g += (long long)seg * ch.C;
    mu += (long long)seg * len;
    ch.start(first, per);
  }
  template <class V>
  __device__ __forceinline__ V at(long long i) const {
    return sub_rn(mul_rn(load_as<V>(y, i), load_as<V>(g + ch.c, 0)), load_as<V>(mu, i));
  }
  __device__ __forceinline__ void next() { ch.next(); }
};

}  // namespace

extern "C" {

int ic_gain_symbolize_seg(const float* y, long long N, long long P, int C, const float* g, const float* mu, int nseg,
                          const int* img, int* img_dev, int* sym, int* kmax_dev, int* kmax_host, void* stream) {
  if (!y || !g || !mu || !img || !img_dev || !sym || !kmax_dev || !kmax_host) return IC_ERR_ARG;
  if (N < 1 || N > 65535 || P < 1 || C < 1 || nseg < 1 || nseg > 65535) return IC_ERR_ARG;
  if (P > 0x7fffffffffffffffll / C / std::max<long long>(N, nseg)) return IC_ERR_ARG;
  for (int m = 0; m < nseg; ++m)
    if (img[m] < 0 || img[m] >= N) return IC_ERR_ARG;
  const bool vec = C % 4 == 0 && aligned16(y) && aligned16(g) && aligned16(mu) && aligned16(sym);
  return seg_symbolize(GainSrc{y, g, mu, img_dev, {C, 0, 0}}, vec, nseg, P * C, img, img_dev, sym, kmax_dev, kmax_host,
                       (hipStream_t)stream);
}

}  // extern "C"

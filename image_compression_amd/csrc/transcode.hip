// Transcoding in the latent domain: the symbols of y at M target qualities from the decoded integers of N source
// streams, in one launch (ic_requant_seg).  Target m names its source img[m]; r and mu1 are the source's decoded
// float integers and its mean, a[img[m]] the source's inverse gains, b[m] the target's gains, mu2[m] the target's
// mean; mu2 and sym are segments of P * C elements back to back:
//     sym[m][i] = symbol_of(sub_rn(mul_rn(mul_rn(add_rn(r[img[m]][i], mu1[img[m]][i]), a[img[m]][c(i)]), b[m][c(i)]), mu2[m][i]))
// The sum is ic_add_mean's one fp32 addition, the two products ic_channel_scale's one fp32 multiplication each, the
// difference ic_codec_symbolize_mean_seg's one fp32 subtraction (fp_rn.h: each rounded once, none contracted with
// another): bit for bit those four calls on the gathered batch, without the gather copy and with neither y_hat nor
// the scaled latent in memory.
// r, mu1, mu2 and sym are dense channels-last storage (P positions, channel fastest; 20 bytes per symbol, the gain rows
// stay in cache).  The walk and the driver are seg_symbolize.h's: 16-byte accesses when every pointer is 16-byte
// aligned and C % 4 == 0 (then every segment and every gain row starts on a 16-byte boundary and a group of four never
// straddles a position).
#include <algorithm>

#include "seg_symbolize.h"

namespace {

struct RequantSrc {
  const float *r, *mu1, *a, *b, *mu2;
  const int* img;
  ChannelCursor ch;
  __device__ __forceinline__ void bind(unsigned seg, long long len, long long first, long long per) {
    const long long src = (long long)img[seg];
    r += src * len;
    mu1 += src * len;
    a += src * ch.C;
    b += (long long)seg * ch.C;
    mu2 += (long long)seg * len;
    ch.start(first, per);
  }
  template <class V>
  __device__ __forceinline__ V at(long long i) const {
    const V y_hat = mul_rn(add_rn(load_as<V>(r, i), load_as<V>(mu1, i)), load_as<V>(a + ch.c, 0));
    return sub_rn(mul_rn(y_hat, load_as<V>(b + ch.c, 0)), load_as<V>(mu2, i));
  }
  __device__ __forceinline__ void next() { ch.next(); }
};

}  // namespace

extern "C" {

int ic_requant_seg(const float* r, const float* mu1, long long N, long long P, int C, const float* a, const float* b,
                   const float* mu2, int nseg, const int* img, int* img_dev, int* sym, int* kmax_dev, int* kmax_host,
                   void* stream) {
  if (!r || !mu1 || !a || !b || !mu2 || !img || !img_dev || !sym || !kmax_dev || !kmax_host) return IC_ERR_ARG;
  if (N < 1 || N > 65535 || P < 1 || C < 1 || nseg < 1 || nseg > 65535) return IC_ERR_ARG;
  if (P > 0x7fffffffffffffffll / C / std::max<long long>(N, nseg)) return IC_ERR_ARG;
  for (int m = 0; m < nseg; ++m)
    if (img[m] < 0 || img[m] >= N) return IC_ERR_ARG;
  const bool vec = C % 4 == 0 && aligned16(r) && aligned16(mu1) && aligned16(a) && aligned16(b) && aligned16(mu2) &&
                   aligned16(sym);
  return seg_symbolize(RequantSrc{r, mu1, a, b, mu2, img_dev, {C, 0, 0}}, vec, nseg, P * C, img, img_dev, sym, kmax_dev,
                       kmax_host, (hipStream_t)stream);
}

}  // extern "C"

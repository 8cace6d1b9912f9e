// Radiance RGBE frames -> fp32 planes (cvvdp_unpack_rgbe, include/cvvdp_hip.h): the device half of the .hdr image input.  The file's
// 4 bytes per pixel cross PCIe; the 12 bytes per pixel the metrics read (CVVDP_F32 blocks) are made here.
//
// Value: float(mantissa) * 2^(E - 136), 0 where E == 0.  A mantissa has 8 bits and the result lies between 2^-135 and 255 * 2^119, so
// it is a fp32 number -- a subnormal one for E < 10 -- for every input: ldexpf is exact, there is nothing to round.
//
// A streaming pass: one thread takes four adjacent pixels with one 16-byte load and writes one 16-byte store per colour plane, a wave
// 1 KiB per instruction.  A frame whose first pixel is not 16-byte aligned on the input or on any of its three output planes (H * W not
// a multiple of 4 and frames packed back to back, odd strides) is taken pixel by pixel with 4-byte accesses, and so are the up to three
// pixels behind the last whole quad of an aligned frame.
#include "kernels.h"

namespace cvvdp {
namespace {

__device__ __forceinline__ void rgbe_pixel(uint32_t w, float& r, float& g, float& b) {
  const int e = (int)(w >> 24);
  const int s = e - 136;
  r = e ? ldexpf((float)(w & 255u), s) : 0.0f;
  g = e ? ldexpf((float)((w >> 8) & 255u), s) : 0.0f;
  b = e ? ldexpf((float)((w >> 16) & 255u), s) : 0.0f;
}

__global__ void __launch_bounds__(kRgbeThreads) k_unpack_rgbe(const RgbeArgs a) {
  const int64_t f = blockIdx.y;
  const uint32_t t = blockIdx.x * (uint32_t)kRgbeThreads + threadIdx.x;
  const uint32_t HW = (uint32_t)a.HW;
  const uint32_t* __restrict__ src = a.src + f * (int64_t)a.HW;
  float* __restrict__ d0 = a.dst + f * a.sf;
  float* __restrict__ d1 = d0 + a.sc;
  float* __restrict__ d2 = d1 + a.sc;
  // the same for every thread of the block
  const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(d0) | reinterpret_cast<uintptr_t>(d1) |
                     reinterpret_cast<uintptr_t>(d2)) & 15u) == 0;
  const uint32_t nq = vec ? HW / 4u : 0u;
  if (t < nq) {                                   // pixels 4t .. 4t+3 < HW
    const uint4 w = reinterpret_cast<const uint4*>(src)[t];
    float4 r, g, b;
    rgbe_pixel(w.x, r.x, g.x, b.x);
    rgbe_pixel(w.y, r.y, g.y, b.y);
    rgbe_pixel(w.z, r.z, g.z, b.z);
    rgbe_pixel(w.w, r.w, g.w, b.w);
    reinterpret_cast<float4*>(d0)[t] = r;
    reinterpret_cast<float4*>(d1)[t] = g;
    reinterpret_cast<float4*>(d2)[t] = b;
  }
  // what the quads leave: every pixel of an unaligned frame, the last H * W % 4 pixels of an aligned one.  4 * nq <= HW < 2^31 and
  // t < 2^31 + 256: the sum fits 32 bits
  const uint32_t i = 4u * nq + t;
  if (i < HW) {
    float r, g, b;
    rgbe_pixel(src[i], r, g, b);
    d0[i] = r;
    d1[i] = g;
    d2[i] = b;
  }
}

}  // namespace

void launch_unpack_rgbe(const RgbeArgs& a, hipStream_t s) {
  // all_vec: H * W / 4 quads per frame and nothing behind them; otherwise one thread per pixel covers both the pixel-by-pixel frames and,
  // on aligned frames, quads and tail
  const uint32_t items = a.all_vec ? (uint32_t)a.HW / 4u : (uint32_t)a.HW;
  const dim3 grid((items + kRgbeThreads - 1) / kRgbeThreads, a.n_frames);
  k_unpack_rgbe<<<grid, kRgbeThreads, 0, s>>>(a);
}

}  // namespace cvvdp

// ---------------------------------------------------------------- C ABI (include/cvvdp_hip.h)
extern "C" {

int cvvdp_unpack_rgbe(cvvdp_handle* h, const void* rgbe, int32_t n_frames, int32_t H, int32_t W, float* out, int64_t stride_c,
                      int64_t stride_f, void* stream) {
  cvvdp::RgbeArgs a;
  if (int rc = cvvdp::rgbe_prepare(h, rgbe, n_frames, H, W, out, stride_c, stride_f, a)) return rc;
  cvvdp::launch_unpack_rgbe(a, static_cast<hipStream_t>(stream));
  return cvvdp::host_check_launch(h, "unpack_rgbe");
}

}  // extern "C"

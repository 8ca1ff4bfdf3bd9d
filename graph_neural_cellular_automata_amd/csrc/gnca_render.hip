// gnca_render.hip — frames and maps as uint8 images (include/gnca.h): the pixel
// work in front of a PNG / video encoder.  Reference: masked_rgb and attn_to_rgb of
// src/testing/test_graph_augmented_regeneration.py:29-47 and save_img of
// src/testing/test_intermediate_loss.py:18-37, which run per frame on the host.
//
// Both kernels write an HWC byte stream whose rows and images are not multiples of 4 bytes in
// general (W = 7, s = 2, rgb: 42 B per row; 5 x 7 x 3 = 105 B per image).  A workgroup owns one
// contiguous byte range of `out` and splits it into a head of < 4 bytes, aligned 32-bit words and a
// tail of < 4 bytes: one lane produces one whole word, consecutive lanes consecutive words, and byte
// stores appear only in the head and the tail.  No atomics: the output is bitwise deterministic.
//
// Built with -ffp-contract=off and correctly rounded division (__graft_entry__.py): the sums are the
// products and additions written here, and the LUT index is bitwise numpy's.

#include "gnca_device.h"

namespace gnca {
namespace {

constexpr int kMaxScale = 16;
constexpr size_t kRenderLdsMax = 60 * 1024;   // the band, its halo rows and the phase tables

__device__ __forceinline__ uint32_t to_byte(float v) {
  v = fminf(fmaxf(v, 0.f), 1.f);            // (a NaN becomes 0)
  return (uint32_t)(int)(v * 255.f);        // truncation
}

// The geometry of one launch, by value.
struct RenderArgs {
  const float* src;
  uint8_t* out;
  long nstride;
  int H, W, s, band, nb;   // band: source rows per workgroup, nb: bands per image
  float thr;
};

// CNT (1 or 4) consecutive bytes of the band's byte stream from byte b (relative to the band's first
// output row), packed little-endian.  pl: the staged planes [CH][rows][W], staged row j = source row
// clamp(r0 - 1 + j); d0 / l1: the per-phase tables.
template <int CH, int CNT>
__device__ __forceinline__ uint32_t render_run(const RenderArgs& a, const float* pl, const int* d0, const float* l1,
                                               int rows, int r0, uint32_t b) {
  const int W = a.W, s = a.s, H = a.H;
  const uint32_t Ws = (uint32_t)W * s;
  uint32_t pix = b / CH;
  int c = (int)(b - pix * CH);
  const uint32_t yb = pix / Ws;               // output row within the band
  int x = (int)(pix - yb * Ws);
  int y = r0 * s + (int)yb;                   // output row within the image
  int qy = y / s, py = y - qy * s;
  int qx = x / s, px = x - qx * s;
  uint32_t word = 0;
#pragma unroll
  for (int k = 0; k < CNT; ++k) {
    int iy0 = qy + d0[py];
    float ly1 = l1[py];
    if (iy0 < 0) { iy0 = 0; ly1 = 0.f; }
    const int iy1 = min(iy0 + 1, H - 1);
    int ix0 = qx + d0[px];
    float lx1 = l1[px];
    if (ix0 < 0) { ix0 = 0; lx1 = 0.f; }
    const int ix1 = min(ix0 + 1, W - 1);
    const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const float* p0 = pl + ((size_t)c * rows + (iy0 - (r0 - 1))) * W;
    const float* p1 = pl + ((size_t)c * rows + (iy1 - (r0 - 1))) * W;
    const float h0 = lx0 * p0[ix0] + lx1 * p0[ix1];
    const float h1 = lx0 * p1[ix0] + lx1 * p1[ix1];
    word |= to_byte(ly0 * h0 + ly1 * h1) << (8 * k);
    if (k + 1 < CNT) {                        // the next byte of the stream
      if (++c == CH) {
        c = 0;
        if (++px == s) { px = 0; ++qx; }
        if (++x == (int)Ws) {
          x = qx = px = 0;
          if (++py == s) { py = 0; ++qy; }
        }
      }
    }
  }
  return word;
}

template <int CH>
__global__ __launch_bounds__(kThreads) void gnca_render(const RenderArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int n = blockIdx.x / a.nb, bi = blockIdx.x - n * a.nb;
  const int H = a.H, W = a.W, s = a.s;
  const int r0 = bi * a.band;
  const int nr = min(a.band, H - r0);         // source rows of this band
  const int rows = nr + 2;                    // with the halo row on each side
  float* pl = lds;
  float* l1 = lds + (size_t)CH * (a.band + 2) * W;
  int* d0 = reinterpret_cast<int*>(l1 + kMaxScale);

  // the s phases of one axis (both axes share them): output q s + p reads source q + d0[p] and the
  // next one with weights 1 - l1[p], l1[p]
  if (tid < s) {
    const float f = ((float)tid + 0.5f) / (float)s - 0.5f;
    d0[tid] = f < 0.f ? -1 : 0;
    l1[tid] = f < 0.f ? 1.f + f : f;
  }
  // stage the band: mask (and, rgb mode, pre-clip) once per source cell
  const size_t HW = (size_t)H * W;
  const float* sn = a.src + (size_t)n * a.nstride;
  const int cells = rows * W;
  for (int e = tid; e < cells; e += kThreads) {
    const int j = e / W, x = e - j * W;
    const int r = min(max(r0 - 1 + j, 0), H - 1);
    const float* p = sn + (size_t)r * W + x;
    const float m = p[3 * HW] > a.thr ? 1.f : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = p[c * HW] * m;
      if (CH == 3) v = fminf(fmaxf(v, 0.f), 1.f);
      pl[(size_t)c * rows * W + e] = v;
    }
    if (CH == 4) pl[(size_t)3 * rows * W + e] = m;
  }
  __syncthreads();

  const size_t pitch = (size_t)W * s * CH;                       // bytes per output row
  const size_t base = ((size_t)n * H * s + (size_t)r0 * s) * pitch;
  const uint32_t len = (uint32_t)((size_t)nr * s * pitch);
  uint8_t* o = a.out + base;
  const uint32_t head = min((uint32_t)((4 - (reinterpret_cast<uintptr_t>(o) & 3)) & 3), len);
  const uint32_t nw = (len - head) >> 2;
  const uint32_t tail = len - head - 4 * nw;
  for (uint32_t w = tid; w < nw; w += kThreads)
    *reinterpret_cast<uint32_t*>(o + head + 4 * (size_t)w) = render_run<CH, 4>(a, pl, d0, l1, rows, r0, head + 4 * w);
  if ((uint32_t)tid < head) o[tid] = (uint8_t)render_run<CH, 1>(a, pl, d0, l1, rows, r0, (uint32_t)tid);
  if ((uint32_t)tid < tail) {
    const uint32_t b = head + 4 * nw + tid;
    o[b] = (uint8_t)render_run<CH, 1>(a, pl, d0, l1, rows, r0, b);
  }
}

// The LUT index of one value (include/gnca.h): lo = the map's min (MINMAX) or 0, den = the divisor,
// ok = whether the map normalises at all.
__device__ __forceinline__ int lut_index(float v, float lo, float den, bool ok, bool clip) {
  float z = ok ? (v - lo) / den : 0.f;
  if (clip) z = fminf(fmaxf(z, 0.f), 1.f);
  return min(max((int)(z * 256.f), 0), 255);
}

template <int CNT>
__device__ __forceinline__ uint32_t colorize_run(const float* m, const uint8_t* lut, float lo, float den, bool ok,
                                                 bool clip, uint32_t b) {
  uint32_t pix = b / 3;
  int c = (int)(b - 3 * pix);
  int idx = lut_index(m[pix], lo, den, ok, clip);
  uint32_t word = 0;
#pragma unroll
  for (int k = 0; k < CNT; ++k) {
    word |= (uint32_t)lut[3 * idx + c] << (8 * k);
    if (k + 1 < CNT && ++c == 3) {
      c = 0;
      idx = lut_index(m[++pix], lo, den, ok, clip);   // (byte k + 1 exists: pix is inside the map)
    }
  }
  return word;
}

__global__ __launch_bounds__(kThreads) void gnca_colorize(int HW, int norm, const float* maps, const uint8_t* lut,
                                                          uint8_t* out) {
  __shared__ uint8_t slut[768];
  __shared__ float red[2][kThreads / 64];
  const int tid = threadIdx.x;
  const float* m = maps + (size_t)blockIdx.x * HW;
  for (int e = tid; e < 768; e += kThreads) slut[e] = lut[e];
  // pass 1: max and min (order-independent, so bitwise reproducible)
  float mx = -INFINITY, mn = INFINITY;
  for (int e = tid; e < HW; e += kThreads) {
    const float v = m[e];
    mx = fmaxf(mx, v);
    mn = fminf(mn, v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, off));
    mn = fminf(mn, __shfl_xor(mn, off));
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = mx;
    red[1][tid >> 6] = mn;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    mx = fmaxf(mx, red[0][w]);
    mn = fminf(mn, red[1][w]);
  }
  const bool minmax = norm == GNCA_NORM_MINMAX;
  const bool ok = minmax ? mx > mn : mx > 0.f;
  const float lo = minmax ? mn : 0.f;
  const float den = minmax ? mx - mn : mx + 1e-8f;
  // pass 2: the bytes (the map is re-read from L2)
  const uint32_t len = 3u * (uint32_t)HW;
  uint8_t* o = out + (size_t)blockIdx.x * len;
  const uint32_t head = min((uint32_t)((4 - (reinterpret_cast<uintptr_t>(o) & 3)) & 3), len);
  const uint32_t nw = (len - head) >> 2;
  const uint32_t tail = len - head - 4 * nw;
  for (uint32_t w = tid; w < nw; w += kThreads)
    *reinterpret_cast<uint32_t*>(o + head + 4 * (size_t)w) = colorize_run<4>(m, slut, lo, den, ok, !minmax, head + 4 * w);
  if ((uint32_t)tid < head) o[tid] = (uint8_t)colorize_run<1>(m, slut, lo, den, ok, !minmax, (uint32_t)tid);
  if ((uint32_t)tid < tail) {
    const uint32_t b = head + 4 * nw + tid;
    o[b] = (uint8_t)colorize_run<1>(m, slut, lo, den, ok, !minmax, b);
  }
}

}  // namespace
}  // namespace gnca

using namespace gnca;

extern "C" int gnca_render_u8(const gnca_render_desc* d, const float* src, uint8_t* out) {
  if (!d || !src || !out || d->N <= 0 || d->H <= 0 || d->W <= 0) return GNCA_ERR_INVALID;
  if (d->upscale < 1 || d->upscale > kMaxScale) return GNCA_ERR_INVALID;
  if (d->mode != GNCA_RENDER_RGB && d->mode != GNCA_RENDER_RGBA) return GNCA_ERR_INVALID;
  if (d->src_nstride < 4 * (int64_t)d->H * d->W || (reinterpret_cast<uintptr_t>(out) & 3)) return GNCA_ERR_INVALID;
  const int ch = d->mode == GNCA_RENDER_RGB ? 3 : 4;
  const size_t tables = kMaxScale * (sizeof(float) + sizeof(int));
  auto lds_of = [&](int band) { return (size_t)ch * (band + 2) * d->W * sizeof(float) + tables; };
  int band = d->H < GNCA_RENDER_BAND_ROWS ? d->H : GNCA_RENDER_BAND_ROWS;
  while (band > 1 && lds_of(band) > kRenderLdsMax) --band;
  if (lds_of(band) > kRenderLdsMax) return GNCA_ERR_UNSUPPORTED;
  // a band's bytes are indexed in 32 bits, the grid in 31
  if ((uint64_t)band * d->upscale * d->W * d->upscale * ch > 0x7fffffffull) return GNCA_ERR_UNSUPPORTED;
  const int64_t nb = (d->H + band - 1) / band;
  if (nb * d->N > 0x7fffffffLL) return GNCA_ERR_INVALID;
  RenderArgs a;
  a.src = src; a.out = out; a.nstride = (long)d->src_nstride;
  a.H = d->H; a.W = d->W; a.s = d->upscale; a.band = band; a.nb = (int)nb;
  a.thr = d->alpha_thr;
  hipStream_t st = reinterpret_cast<hipStream_t>(d->stream);
  const dim3 grid((unsigned)(nb * d->N));
  if (ch == 3) hipLaunchKernelGGL(gnca_render<3>, grid, dim3(kThreads), lds_of(band), st, a);
  else hipLaunchKernelGGL(gnca_render<4>, grid, dim3(kThreads), lds_of(band), st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

extern "C" int gnca_colorize_u8(const gnca_colorize_desc* d, const float* maps, const uint8_t* lut, uint8_t* out) {
  if (!d || !maps || !lut || !out || d->N <= 0 || d->H <= 0 || d->W <= 0) return GNCA_ERR_INVALID;
  if (d->norm != GNCA_NORM_MAX && d->norm != GNCA_NORM_MINMAX) return GNCA_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(out) & 3) return GNCA_ERR_INVALID;
  if ((int64_t)d->H * d->W > 0x7fffffffLL / 3) return GNCA_ERR_UNSUPPORTED;   // a map's bytes are indexed in 32 bits
  hipLaunchKernelGGL(gnca_colorize, dim3((unsigned)d->N), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(d->stream),
                     d->H * d->W, d->norm, maps, lut, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

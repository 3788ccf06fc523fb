// fl_frontend.hip -- gfx950 kernels for the quantisation front-end of cup_linemod
// (reference: linemod/linemod.cpp:230-385 quantizedOrientations + hysteresisGradient,
//  :434-453 ColorGradientPyramid::pyrDown, :567-685 quantizedNormals, :721-739 NN downsample).
//
//   k_color_quantize   GaussianBlur 7x7 -> Sobel x/y -> max-magnitude channel -> fastAtan2 ->
//                      16-bin quantise -> 3x3 majority vote, fused in registers (sliding window per
//                      column, wave shuffles for x+-1): the BGR image is read from HBM once and only
//                      the one-hot byte image is written.
//   k_pyrdown_pairs    cv::pyrDown [1 4 6 4 1]^2, (acc+128)>>8, REFLECT_101, border pairs included (k_pyrdown_general:
//                      sizes the pair kernel does not take)
//   k_depth_quantize   bilateral 8-neighbour LSQ normal (int64) + NORMAL_LUT + exact 5x5 median of the
//                      one-hot codes (replicated border), fused in registers like k_color_quantize; at even sizes it
//                      also writes the half-size image src(2y, 2x) of the next pyramid level
//   k_resize_nn_half   src(2y, 2x) for the levels after that, and for level 1 at other sizes
// Both quantisers walk chunks of rows whose height a whole-image launch picks from the batch size (fl_eager_chunk_rows).
//
// The integer stages are exact; the float stages restate OpenCV 3.x's arithmetic operator by
// operator (built with -ffp-contract=off; IEEE divide/sqrt are hipcc's default, and the quantisers' square root, reciprocal
// and quotient are those operations without their range handling: fl_ranged_math.h), so they equal
// oracle/frontend_oracle.c bit for bit.  OpenCV itself is not available to compare with:
// "parity unpinned" at this boundary.
#include "fl_internal.h"
#include "fl_ranged_math.h"
#include <float.h>
#include <type_traits>

#ifndef FL_CQ_DOT4
#define FL_CQ_DOT4 1               // horizontal blur taps by v_dot4_u32_u8 against constant weight words
#endif

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int reflect101(int p, int len)
{
  if (len == 1) return 0;
  while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

// cv::fastAtan2 in degrees (OpenCV 3.x hal::fastAtan32f), used by cv::phase (linemod.cpp:303)
__device__ __forceinline__ float fast_atan2_deg(float y, float x)
{
  const float p1 = 0.9997878412794807f * (float)(180 / 3.14159265358979323846);
  const float p3 = -0.3258083974640975f * (float)(180 / 3.14159265358979323846);
  const float p5 = 0.1555786518463281f * (float)(180 / 3.14159265358979323846);
  const float p7 = -0.04432655554792128f * (float)(180 / 3.14159265358979323846);
  const float ax = fabsf(x), ay = fabsf(y);
  // ax >= ay: c = ay / (ax + eps), a = poly(c); else c = ax / (ay + eps), a = 90 - poly(c) -- the same operations on swapped
  // operands, so one division and one polynomial serve both (as two branches a wave with lanes of both kinds ran each in turn)
  const bool steep = !(ax >= ay);
  // (div_rn: the correctly rounded quotient without the range handling of `/`; the operands are inside its stated domain)
  const float c = div_rn(steep ? ax : ay, (steep ? ay : ax) + (float)DBL_EPSILON);
  const float c2 = c * c;
  const float poly = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  float a = steep ? 90.f - poly : poly;
  if (x < 0) a = 180.f - a;
  if (y < 0) a = 360.f - a;
  return a;
}

// ------------------------------------------------------------------------------------------
// k_color_quantize: one wavefront owns a strip of 64 adjacent image columns (60 outputs plus two
// halo columns on each side) and walks chunk_rows output rows downwards with the whole filter chain in
// registers: a 7-row ring of horizontal-blur sums per channel, 3-row rings of the smoothed pixel
// (packed B|G<<8|R<<16) and of the 16-bin code for x-1, x, x+1 -- horizontal neighbours come from
// wave shuffles, vertical ones from the rings.  No LDS, no barriers; every source byte is fetched
// once per strip (plus the 4-column / 10-row halo) through two wide loads per row and lane.
// chunk_rows is CQ_CH for a tiled (lazy) launch, whose chunks are the tile rows; a whole-image launch takes 120-row chunks
// where the batch still fills the device with them (fl_eager_chunk_rows): every chunk recomputes 10 blur rows, 4 smoothed
// rows and 2 Sobel rows of halo for its first output row.
#define CQ_COLS 60
#define CQ_CH 60

// Neighbour lanes by whole-wave DPP shifts (gfx9 wave_shr:1 / wave_shl:1): one v_mov_dpp instead of the
// ds_bpermute + index arithmetic of __shfl_up / __shfl_down.  Lane 0 / lane 63, which have no such neighbour, receive 0
// (bound_ctrl): keeping their own value, as those do, costs a copy of v into the destination ahead of every shift, and nothing
// that either quantiser stores depends on what these lanes get (see the callers).
__device__ __forceinline__ unsigned wave_from_prev0(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, true); }
__device__ __forceinline__ unsigned wave_from_next0(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xF, 0xF, true); }

// The 7-pixel window of a lane, fetched as 4-byte aligned dwords (a 16-byte load costs 28-32 cycles per wave-instruction at
// 4-byte alignment and 70-76 at byte alignment or a 3-byte lane stride: tools/probes/ldwidth.hip).
// The window starts at pixel first = clamp(xc - 3, 0, w - 7), i.e. it lies inside the row for every lane of an image at
// least 7 wide; its 21 bytes begin row_mis + 3 * first bytes behind the row's address rounded down to a multiple of 4
// (row_mis: the row address's low two bits).  Whatever that sum's low two bits are, the 21 bytes lie inside the six aligned
// dwords from *off on, the first of which holds the window's first byte and the last of which its byte 20 - shift: no dword
// without a byte of the window is read, so nothing in front of a frame's first row or behind its last one is touched.
// *shift is what v_alignbyte_b32 takes to move the window to byte 0.
__host__ __device__ __forceinline__ void cq_window_addr(uint32_t row_mis, int w, int xc, uint32_t *off, uint32_t *shift, int *first)
{
  const int f = xc - 3 < 0 ? 0 : (xc - 3 > w - 7 ? w - 7 : xc - 3);
  const uint32_t o = row_mis + 3u * (uint32_t)f;
  *off = o & ~3u;
  *shift = o & 3u;
  *first = f;
}

// ({hi, lo} >> 8 * (s & 3)), low dword: v_alignbyte_b32
__host__ __device__ __forceinline__ uint32_t cq_alignbyte(uint32_t hi, uint32_t lo, uint32_t s)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, s);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (s & 3u)));
#endif
}

// wd[0..5]: bytes 3 t + ch of it are tap t (column clamp(xc + t - 3, 0, w - 1), BORDER_REPLICATE) of channel ch; bytes 21..23
// are not defined.  row4 is the row's address rounded down to a multiple of 4.  Two loads in every lane.  The lanes within 3
// columns of an image edge (and the ones beside the image, whose xc is the edge column) have dpx = xc - 3 - first != 0: their
// taps are the window moved by dpx pixels with the edge pixel repeated.  The waves that hold such lanes (any_left / any_right,
// wave-uniform) rebuild it: the edge pixel's three bytes continue the window as a 12-byte pattern of period 3 on that side, and
// every lane takes its six dwords out of that stream at byte 12 + 3 dpx (left) or 3 dpx (right) -- a select per bit of the dword
// index and an alignbyte; lanes with dpx == 0 keep their window.
__host__ __device__ __forceinline__ void cq_window(const uint8_t *__restrict__ row4, uint32_t row_mis, int w, int xc, bool any_left,
                                                   bool any_right, uint32_t *wd)
{
  uint32_t off, shift;
  int first;
  cq_window_addr(row_mis, w, xc, &off, &shift, &first);
  const int dpx = xc - 3 - first;
  uint32_t d[6];
  const uint8_t *q = (const uint8_t *)__builtin_assume_aligned(row4 + off, 4);
  __builtin_memcpy(d, q, 16);
  __builtin_memcpy(d + 4, q + 16, 8);
#pragma unroll
  for (int k = 0; k < 5; ++k) wd[k] = cq_alignbyte(d[k + 1], d[k], shift);
  wd[5] = cq_alignbyte(d[5], d[5], shift);                // byte 20 of the window arrives; 21..23 carry no tap
  // (the selects are written out on named values: over arrays the compiler turns them into indexed loads from scratch)
#define CQ_TAKE(e0, e1, e2, e3, e4, e5, e6, e7, e8)                                                                                 \
  {                                                                                                                                 \
    const bool b0 = (dw & 1u) != 0u, b1 = (dw & 2u) != 0u;                                                                          \
    const uint32_t t0 = b0 ? e1 : e0, t1 = b0 ? e2 : e1, t2 = b0 ? e3 : e2, t3 = b0 ? e4 : e3, t4 = b0 ? e5 : e4, t5 = b0 ? e6 : e5, \
                   t6 = b0 ? e7 : e6, t7 = b0 ? e8 : e7;                                                                            \
    const uint32_t g0 = b1 ? t2 : t0, g1 = b1 ? t3 : t1, g2 = b1 ? t4 : t2, g3 = b1 ? t5 : t3, g4 = b1 ? t6 : t4, g5 = b1 ? t7 : t5; \
    wd[0] = cq_alignbyte(g1, g0, s);                                                                                                \
    wd[1] = cq_alignbyte(g2, g1, s);                                                                                                \
    wd[2] = cq_alignbyte(g3, g2, s);                                                                                                \
    wd[3] = cq_alignbyte(g4, g3, s);                                                                                                \
    wd[4] = cq_alignbyte(g5, g4, s);                                                                                                \
    wd[5] = cq_alignbyte(g5, g5, s);                                                                                                \
  }
  if (any_left) {
    const uint32_t s = dpx < 0 ? (uint32_t)-dpx : 0u, dw = 3u - s;         // stream byte 12 - 3 s = dword 3 - s, byte s
    const uint32_t p = wd[0] & 0xFFFFFFu;                                  // pixel 0: B | G << 8 | R << 16
    // stream bytes 0..11: B G R B | G R B G | R B G R, then the window
    CQ_TAKE((p | (p << 24)), ((p >> 8) | (p << 16)), ((p >> 16) | (p << 8)), wd[0], wd[1], wd[2], wd[3], wd[4], wd[5])
  }
  if (any_right) {
    const uint32_t n = dpx > 0 ? 3u * (uint32_t)dpx : 0u, dw = n >> 2, s = n & 3u;     // stream byte 3 dpx = dword dw, byte s
    const uint32_t p = (wd[4] >> 16) | ((wd[5] & 0xFFu) << 16);            // pixel 6 (bytes 18..20)
    // the window, whose bytes 20..31 become R B G R | B G R B | G R B G (the ninth dword is read by no lane: dw <= 2)
    CQ_TAKE(wd[0], wd[1], wd[2], wd[3], wd[4], ((p >> 16) | (p << 8)), (p | (p << 24)), ((p >> 8) | (p << 16)), 0u)
  }
#undef CQ_TAKE
}

// Horizontal [8 28 56 72 56 28 8] sums of a row's three channels at column xc.  kNarrow (w < 8): a tap at a time.
template <bool kNarrow>
__device__ __forceinline__ void cq_hrow(const uint8_t *__restrict__ src, int w, int h, int row, int xc, bool any_left, bool any_right,
                                        int *h3)
{
  const int kk[7] = {8, 28, 56, 72, 56, 28, 8};
  const uint8_t *p = src + (size_t)clampi(row, 0, h - 1) * (size_t)(w * 3);          // wave-uniform: scalar arithmetic
  int a0 = 0, a1 = 0, a2 = 0;
  if (!kNarrow) {
    const uint32_t mis = (uint32_t)(uintptr_t)p & 3u;
    uint32_t wd[6];
    cq_window(p - mis, mis, w, xc, any_left, any_right, wd);
    // the 7 taps of a channel sit at bytes 3 t + ch of the 24-byte window: per dword one v_dot4_u32_u8 against a constant
    // word that holds the tap weights at this channel's byte positions (0 elsewhere) -- 6 dot products per channel instead of
    // 7 byte extractions + 7 multiply-adds; integer arithmetic, the same sums (<= 255 * 256)
#if FL_CQ_DOT4
    unsigned acc[3] = {0u, 0u, 0u};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        unsigned wk = 0;
#pragma unroll
        for (int t = 0; t < 7; ++t)
          if (((3 * t + ch) >> 2) == k) wk |= (unsigned)kk[t] << (8 * ((3 * t + ch) & 3));
        if (wk != 0u) acc[ch] = __builtin_amdgcn_udot4(wd[k], wk, acc[ch], false);     // (dword 5 holds a tap of channel 2 only)
      }
    a0 = (int)acc[0]; a1 = (int)acc[1]; a2 = (int)acc[2];
#else
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      const int b0 = 3 * t, b1 = 3 * t + 1, b2 = 3 * t + 2;
      a0 += kk[t] * (int)((wd[b0 >> 2] >> (8 * (b0 & 3))) & 0xFFu);
      a1 += kk[t] * (int)((wd[b1 >> 2] >> (8 * (b1 & 3))) & 0xFFu);
      a2 += kk[t] * (int)((wd[b2 >> 2] >> (8 * (b2 & 3))) & 0xFFu);
    }
#endif
  } else {
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      const uint8_t *q = p + 3 * clampi(xc + t - 3, 0, w - 1);       // BORDER_REPLICATE
      a0 += kk[t] * q[0];
      a1 += kk[t] * q[1];
      a2 += kk[t] * q[2];
    }
  }
  h3[0] = a0;
  h3[1] = a1;
  h3[2] = a2;
}

// for tests/test_cq_window_cpu.py (host arithmetic, no GPU): the window addressing, and the taps cq_window makes of a row
extern "C" void fl_dev_cq_window_addr(unsigned row_mis, int w, int xc, unsigned *off, unsigned *shift, int *first)
{
  cq_window_addr(row_mis, w, xc, off, shift, first);
}
extern "C" void fl_dev_cq_window_taps(const uint8_t *row4, unsigned row_mis, int w, int xc, int any_left, int any_right, uint8_t *taps21)
{
  uint32_t wd[6];
  cq_window(row4, row_mis, w, xc, any_left != 0, any_right != 0, wd);
  for (int b = 0; b < 21; ++b) taps21[b] = (uint8_t)(wd[b >> 2] >> (8 * (b & 3)));
}

#ifndef FL_CQ_WPE
#define FL_CQ_WPE 6              // 6 waves per SIMD (measured: 5 -> 6 gives -2 % front-end time).  The kernel now holds 58 VGPRs: 7 and 8
                                 // fit without spills and were measured at 0 / -0.09 ms (level 1 / tiled level 0), profiles/README.md
#endif
// kMag (template extraction): frame z's squared gradient magnitude goes to mag_out + z * out_stride floats, i.e. the
// magnitude images have the quantised images' pitch in elements.  The front-end of the recognition path launches
// k_color_quantize<false>, whose mag_out is null there.
// The 7-row ring trades roles by unrolling: seven steps make the loop body, step P writes the new source row into slot P and
// reads the window from slot P + 1 on, so no row is moved.  Virtual rows above the image's first row and below its last one
// have the window of that row (the window does not advance there): those steps, at most two at either end, push the
// smoothed pixels of the step before into the 3-row rings again.
template <bool kMag, bool kNarrow>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kNarrow ? 6 : FL_CQ_WPE, kNarrow ? 6 : FL_CQ_WPE))) void k_color_quantize(const uint8_t *__restrict__ bgr, size_t in_stride,
                                                        uint8_t *__restrict__ dst, size_t out_stride, int w, int h,
                                                        float threshold_sq, int nstrips, int nchunks, int chunk_rows,
                                                        float *__restrict__ mag_out, const uint32_t *__restrict__ tiles,
                                                        size_t tiles_stride)
{
  // the wave index is the same in all 64 lanes: as a scalar it keeps the strip, the rows and the row addresses on the scalar unit
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + wave;
  if (item >= nstrips * nchunks) return;
  const int strip = item % nstrips, chunk = item / nstrips;
  int row_lo = 0, row_hi = h - 1;
  if (tiles) {             // lazy fine level: only the tiles (and, inside a tile, the rows) some candidate's spreads read
    const uint32_t *tb = tiles + (size_t)blockIdx.z * tiles_stride;
    const int t = chunk * nstrips + strip;
    if (!((tb[FL_TILE_WORDS + (t >> 5)] >> (t & 31)) & 1u)) return;                          // wave-uniform
    const uint32_t rw = tb[2 * FL_TILE_WORDS + 32 * FL_TILE_WORDS + t];
    row_lo = (int)(rw >> 16);
    row_hi = (int)(rw & 0xFFFFu);
  }
  const uint8_t *src = bgr + (size_t)blockIdx.z * in_stride;
  uint8_t *out = dst + (size_t)blockIdx.z * out_stride;
  const int x = strip * CQ_COLS + lane - 2;
  // a sample requested outside the image is the sample at the clamped position -- for the blur's own
  // taps and for Sobel's BORDER_REPLICATE on the *smoothed* image alike (linemod.cpp:247-249)
  const int xc = clampi(x, 0, w - 1);
  const int y0 = max(chunk * chunk_rows, row_lo), y1 = min(min(h, chunk * chunk_rows + chunk_rows), row_hi + 1);
  if (y0 >= y1) return;                                  // no row to write
  // the waves that hold lanes within 3 columns of an image edge (lane 0 is column strip * CQ_COLS - 2, lane 63 + 61)
  const bool any_left = strip == 0, any_right = strip * CQ_COLS + 61 > w - 4;

  int H[7][3];
  {
    const int center = clampi(y0 - 2, 0, h - 1);
#pragma unroll
    for (int i = 0; i < 7; ++i) cq_hrow<kNarrow>(src, w, h, center + i - 3, xc, any_left, any_right, H[i]);
  }
  uint32_t Sl[3] = {0, 0, 0}, Sc[3] = {0, 0, 0}, Sr[3] = {0, 0, 0};
  uint32_t Qp[3] = {0, 0, 0};
  float Mg[3] = {0.f, 0.f, 0.f};
  // vertical pass over the window whose first row is in slot p + the single rounding of the 8-bit GaussianBlur:
  // (acc + 2^15) >> 16.  H <= 255 * 256, so every product fits 24 bits: __umul24 is a full-rate multiply where the generic
  // 32-bit one runs at quarter rate; the kernel is symmetric, so 4 multiplies per channel instead of 7.  The smoothed pixel
  // (B | G << 8 | R << 16) and its neighbours' enter the 3-row rings.
  auto smooth = [&](int p) __attribute__((always_inline)) {
    uint32_t vv[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      vv[ch] = __umul24(8u, (unsigned)(H[p % 7][ch] + H[(p + 6) % 7][ch])) + __umul24(28u, (unsigned)(H[(p + 1) % 7][ch] + H[(p + 5) % 7][ch])) +
               __umul24(56u, (unsigned)(H[(p + 2) % 7][ch] + H[(p + 4) % 7][ch])) + __umul24(72u, (unsigned)H[(p + 3) % 7][ch]);
    const uint32_t S = (uint32_t)(((int)vv[0] + (1 << 15)) >> 16) | ((uint32_t)(((int)vv[1] + (1 << 15)) >> 16) << 8) |
                       ((uint32_t)(((int)vv[2] + (1 << 15)) >> 16) << 16);
    // lanes 0 and 63 have no such neighbour: what they get reaches their own label only, which feeds the votes of lanes 0, 1
    // and 62, 63 -- halo lanes that store nothing
    const uint32_t L = wave_from_prev0(S), R = wave_from_next0(S);
    Sl[0] = Sl[1]; Sl[1] = Sl[2]; Sl[2] = L;
    Sc[0] = Sc[1]; Sc[1] = Sc[2]; Sc[2] = S;
    Sr[0] = Sr[1]; Sr[1] = Sr[2]; Sr[2] = R;
  };
  auto again = [&]() __attribute__((always_inline)) {     // a virtual row outside the image: the smoothed row of the step before
    Sl[0] = Sl[1]; Sl[1] = Sl[2];
    Sc[0] = Sc[1]; Sc[1] = Sc[2];
    Sr[0] = Sr[1]; Sr[1] = Sr[2];
  };
  // what follows the smoothed row of virtual row yv: Sobel at yv - 1, the vote and the store at yv - 2
  auto finish = [&](int yv) __attribute__((always_inline)) {
    if (yv < y0) return;                               // wave-uniform
    // Sobel 3x3 at row ys = yv - 1 (rings hold virtual rows ys-1, ys, ys+1), strongest channel,
    // fastAtan2, 16 bins (:248-303, :314)
    const int ys = yv - 1;
    int bdx = 0, bdy = 0, bmag = 0;
    {
      int dxs[3], dys[3], mags[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int sh = 8 * ch;
#define PX(v) ((int)(((v) >> sh) & 0xFFu))
        const int dx = (PX(Sr[0]) - PX(Sl[0])) + 2 * (PX(Sr[1]) - PX(Sl[1])) + (PX(Sr[2]) - PX(Sl[2]));
        const int dy = (PX(Sl[2]) - PX(Sl[0])) + 2 * (PX(Sc[2]) - PX(Sc[0])) + (PX(Sr[2]) - PX(Sr[0]));
#undef PX
        dxs[ch] = dx;
        dys[ch] = dy;
        mags[ch] = __mul24(dx, dx) + __mul24(dy, dy);      // |dx|, |dy| <= 1020: the full-rate 24-bit multiply
      }
      if (mags[0] >= mags[1] && mags[0] >= mags[2]) { bdx = dxs[0]; bdy = dys[0]; bmag = mags[0]; }
      else if (mags[1] >= mags[0] && mags[1] >= mags[2]) { bdx = dxs[1]; bdy = dys[1]; bmag = mags[1]; }
      else { bdx = dxs[2]; bdy = dys[2]; bmag = mags[2]; }
    }
    const float ang = fast_atan2_deg((float)bdy, (float)bdx);
    int qi = __float2int_rn(ang * (float)(16.0 / 360.0));        // cvRound: round half to even
    qi = qi < 0 ? 0 : (qi > 255 ? 255 : qi);
    // hysteresisGradient :316-335: border rows/cols zeroed, interior folded to 8 bins
    const bool inside = ys > 0 && ys < h - 1 && x > 0 && x < w - 1;
    // the vote counts the labels of the 3x3 neighbourhood in eight 4-bit counters; each pixel contributes the
    // counter word of its own label, the row sum x-1, x, x+1 is formed once and kept for three rows
    const uint32_t q = inside ? (uint32_t)(qi & 7) : 0u;
    const uint32_t oh = 1u << (4 * q);
    const uint32_t ohl = wave_from_prev0(oh), ohr = wave_from_next0(oh);
    Qp[0] = Qp[1]; Qp[1] = Qp[2]; Qp[2] = oh + ohl + ohr;
    Mg[0] = Mg[1]; Mg[1] = Mg[2]; Mg[2] = (float)bmag;
    if (yv < y0 + 2) return;
    // 3x3 majority vote at row yo = yv - 2 (:337-384)
    const int yo = yv - 2;
    if (lane >= 2 && lane < 2 + CQ_COLS && x < w && yo < y1) {
      uint8_t res = 0;
      if (yo >= 1 && yo < h - 1 && x >= 1 && x < w - 1 && Mg[1] > threshold_sq) {
        // :337-384: the first label with the most votes wins if it has >= 5 of the 9 -- a strict majority, so it
        // is the only counter >= 5: adding 3 to every counter (max 9 + 3, no carry) sets bit 3 exactly there
        const unsigned hist = Qp[0] + Qp[1] + Qp[2];       // 8 x 4-bit counters
        const unsigned maj = (hist + 0x33333333u) & 0x88888888u;
        if (maj) res = (uint8_t)(1u << ((__ffs((int)maj) - 4) >> 2));
      }
      out[(size_t)yo * w + x] = res;
      // template extraction also wants the squared magnitude image (linemod.cpp:461-513)
      if (kMag) mag_out[(size_t)blockIdx.z * out_stride + (size_t)yo * w + x] = Mg[1];
      else if (mag_out) mag_out[(size_t)yo * w + x] = Mg[1];
    }
  };

  // virtual rows y0 - 2 .. y1 + 1.  The first one has the window that was just loaded; rows <= 0 keep it; rows 1 .. h - 1 take
  // one new source row each; rows >= h keep the last window.
  const int ylast = y1 + 1, yadv = min(ylast, h - 1);
  int yv = y0 - 2;
  smooth(0);                                             // yv < y0: nothing follows
  for (++yv; yv <= min(ylast, 0); ++yv) {
    again();
    finish(yv);
  }
  for (;;) {
#pragma unroll
    for (int P = 0; P < 7; ++P) {
      if (yv > yadv) goto below;
      cq_hrow<kNarrow>(src, w, h, yv + 3, xc, any_left, any_right, H[P]);
      smooth(P + 1);
      finish(yv);
      ++yv;
    }
  }
below:
  for (; yv <= ylast; ++yv) {
    again();
    finish(yv);
  }
}

int fl_launch_quantized_orientations(fl_context *ctx, const uint8_t *bgr, size_t in_stride, uint8_t *dst,
                                     size_t out_stride, int n_frames, int w, int h, float weak_threshold)
{
  return fl_launch_quantized_orientations_mag(ctx, bgr, in_stride, dst, out_stride, n_frames, w, h, weak_threshold, nullptr);
}

// Chunk height of a whole-image (eager) quantiser launch: 120 rows where the launch then still has FL_CHUNK_FILL times the
// waves the device holds at once, else 60 (so the small-batch launches are what they were).  Measured at 4096 VGA frames
// (profiles/README.md): 120 rows beat 60; 240 rows and whole images, which leave the level-1 colour launch 4 and 2 rounds of
// long waves, were slower again and are not chosen.  Option frontend_chunk_rows != 0 forces a height.
#define FL_CHUNK_FILL 4
template <typename K>
static long waves_per_cu(K kernel, long *cache)
{
  if (*cache == 0) {
    int blocks = 0;
    *cache = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kernel, 256, 0) == hipSuccess && blocks > 0 ? 4l * blocks : 32;
  }
  return *cache;
}
static int fl_eager_chunk_rows(const fl_context *ctx, long per_cu, int nstrips, int n_frames, int h)
{
  if (ctx->opt.frontend_chunk_rows) return (int)ctx->opt.frontend_chunk_rows;
  const long need = (long)FL_CHUNK_FILL * ctx->cus * per_cu;
  return h > 60 && (long)nstrips * n_frames * ((h + 119) / 120) >= need ? 120 : 60;
}

static_assert(CQ_COLS == FL_TILE && CQ_CH == FL_TILE, "the lazy tile grid is k_color_quantize's work decomposition");
static int launch_color_quantize(fl_context *ctx, const uint8_t *bgr, size_t in_stride, uint8_t *dst, size_t out_stride, int n_frames,
                                 int w, int h, float weak_threshold, float *mag_out, const uint32_t *tiles, size_t tiles_stride)
{
  static long per_cu[4] = {0, 0, 0, 0};
  const int nstrips = (w + CQ_COLS - 1) / CQ_COLS;
  const bool narrow = w < 8;                             // no 7-pixel window inside a row to load: a tap at a time
  auto launch = [&](auto kernel, long *cache) {
    const int rows = tiles ? CQ_CH : fl_eager_chunk_rows(ctx, waves_per_cu(kernel, cache), nstrips, n_frames, h);
    const int nchunks = (h + rows - 1) / rows;
    dim3 grid((nstrips * nchunks + 3) / 4, 1, n_frames);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, bgr, in_stride, dst, out_stride, w, h, weak_threshold * weak_threshold,
                       nstrips, nchunks, rows, mag_out, tiles, tiles_stride);
  };
  if (mag_out) {
    if (narrow) launch(k_color_quantize<true, true>, &per_cu[3]);
    else launch(k_color_quantize<true, false>, &per_cu[1]);
  } else {
    if (narrow) launch(k_color_quantize<false, true>, &per_cu[2]);
    else launch(k_color_quantize<false, false>, &per_cu[0]);
  }
  FL_HIP(ctx, hipGetLastError());
  return FL_OK;
}

int fl_launch_quantized_orientations_mag(fl_context *ctx, const uint8_t *bgr, size_t in_stride, uint8_t *dst,
                                         size_t out_stride, int n_frames, int w, int h, float weak_threshold, float *mag_out)
{
  return launch_color_quantize(ctx, bgr, in_stride, dst, out_stride, n_frames, w, h, weak_threshold, mag_out, nullptr, 0);
}

// ------------------------------------------------------------------------------------------
// cv::pyrDown.  The stage is bound by vector-memory instructions, whose cost on gfx950 depends on alignment and lane
// stride much more than on width (tools/probes/ldwidth.hip: a 16-byte load costs ~30 cycles per wave when 4-byte
// aligned, ~70 at byte alignment or a 6-byte lane stride; a byte load at stride 5 ~25).  So:
//   k_pyrdown_pairs   one thread makes TWO adjacent output pixels; their 7 source pixels are 21 bytes
//                     inside the 4-byte aligned 24-byte window starting at 12 x' - 8 -> one 16-byte + one 8-byte
//                     aligned load per source row, three 2-byte stores per thread.  The first and the last pair of a
//                     row load at shifted, in-range addresses of the same alignment and rebuild their reflected
//                     window with a few selects (a second launch of one thread per border pixel, 75 byte loads each,
//                     used to take a third of this kernel's time)
//   k_pyrdown_general any pixel, REFLECT_101 taps fetched one by one: whole images the pair kernel does not take
//                     (dw < 8, odd w or dw)
__device__ __forceinline__ void pyrdown_general_px(const uint8_t *__restrict__ src, int w, int h, int x, int y, uint8_t *o)
{
  const int k[5] = {1, 4, 6, 4, 1};
  int acc0 = 0, acc1 = 0, acc2 = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int yy = reflect101(2 * y + j - 2, h);
    int r0 = 0, r1 = 0, r2 = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int xx = reflect101(2 * x + i - 2, w);
      const uint8_t *p = src + ((size_t)yy * w + xx) * 3;
      r0 += k[i] * p[0];
      r1 += k[i] * p[1];
      r2 += k[i] * p[2];
    }
    acc0 += k[j] * r0;
    acc1 += k[j] * r1;
    acc2 += k[j] * r2;
  }
  o[0] = (uint8_t)((acc0 + 128) >> 8);
  o[1] = (uint8_t)((acc1 + 128) >> 8);
  o[2] = (uint8_t)((acc2 + 128) >> 8);
}

__global__ __launch_bounds__(256) void k_pyrdown_general(const uint8_t *__restrict__ src_, size_t in_stride,
                                                         uint8_t *__restrict__ dst_, size_t out_stride, int w, int h)
{
  const int dw = w / 2, dh = h / 2;
  const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (x >= dw || y >= dh) return;
  const uint8_t *src = src_ + (size_t)blockIdx.z * in_stride;
  uint8_t *dst = dst_ + (size_t)blockIdx.z * out_stride;
  pyrdown_general_px(src, w, h, x, y, dst + ((size_t)y * dw + x) * 3);
}

// A wave owns 64 pairs of adjacent output pixels and walks PD_ROWS output rows down: output row y reads source rows
// 2y - 2 .. 2y + 2 and shares three of them with row y + 1, so the horizontal sums of a source row (six per lane: two pixels x
// three channels) are formed once and kept in a five-row register ring that trades roles by unrolling (two new source rows
// per output row instead of five, 140 vector instructions per output row instead of 312; measured: front-end 4.96 -> 4.87 ms
// per 2048 VGA frames).
#define PD_ROWS 8
__global__ __launch_bounds__(256) void k_pyrdown_pairs(const uint8_t *__restrict__ src_, size_t in_stride,
                                                       uint8_t *__restrict__ dst_, size_t out_stride, int w, int h)
{
  const int dw = w / 2, dh = h / 2, np = dw / 2;          // np pairs per output row, dealt evenly over the row's waves
  const int per = (np + (int)gridDim.x - 1) / (int)gridDim.x, lane = threadIdx.x & 63;
  const int xp = blockIdx.x * per + lane;
  const int y0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * PD_ROWS;
  if (lane >= per || xp >= np || y0 >= dh) return;
  const uint8_t *src = src_ + (size_t)blockIdx.z * in_stride;
  uint8_t *dst = dst_ + (size_t)blockIdx.z * out_stride;
  // The first and the last pair of a row (w is even here) have taps outside the row.  They load in-range bytes instead and
  // rebuild the REFLECT_101 window in registers, in the waves that hold them (wave-uniform tests), with selects:
  //   first: source pixels -2, -1 are pixels 2, 1.  Row bytes 0..15 go to window bytes 8..23, bytes 2..7 are put together
  //          from pixels 2 and 1 (row bytes 6..8 and 3..5).
  //   last:  source pixel w is pixel w - 2, i.e. window bytes 20..22 repeat bytes 14..16; the 8-byte load would end 4 bytes
  //          past the row, so it starts 4 bytes earlier and only its upper half is used.
  const bool first = xp == 0, last = xp == np - 1;
  const bool wave_first = blockIdx.x == 0, wave_last = blockIdx.x == gridDim.x - 1;
  const int off16 = first ? 0 : 12 * xp - 8, off8 = first ? 16 : (last ? 12 * xp + 4 : 12 * xp + 8);
  // horizontal [1 4 6 4 1] sums of one source row for this lane's two output pixels (taps 0..4 and 2..6 of the seven source
  // pixels 4 xp - 2 .. 4 xp + 4; bytes 12 xp - 8 .. 12 xp + 15 hold them from byte 2 on)
  auto hrow = [&](int r, int (&o)[6]) {
    const int yy = reflect101(r, h);
    uint32_t wd[6];
    const uint8_t *p = src + (size_t)yy * w * 3;
    __builtin_memcpy(wd, p + off16, 16);
    __builtin_memcpy(wd + 4, p + off8, 8);
    if (wave_first) {
      const uint32_t mix = (wd[2] & 0xFFu) | ((wd[0] >> 24) << 8) | (wd[1] << 16);
      const uint32_t n0 = wd[1], n2 = wd[0], n3 = wd[1], n4 = wd[2], n5 = wd[3];
      wd[0] = first ? n0 : wd[0];
      wd[1] = first ? mix : wd[1];
      wd[2] = first ? n2 : wd[2];
      wd[3] = first ? n3 : wd[3];
      wd[4] = first ? n4 : wd[4];
      wd[5] = first ? n5 : wd[5];
    }
    if (wave_last) {
      const uint32_t hi = wd[5];
      wd[4] = last ? hi : wd[4];
      wd[5] = last ? ((wd[3] >> 16) | (hi << 16)) : wd[5];
    }
#define SB(b) ((int)((wd[(b) >> 2] >> (8 * ((b) & 3))) & 0xFFu))
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      o[ch] = SB(2 + ch) + 4 * SB(5 + ch) + 6 * SB(8 + ch) + 4 * SB(11 + ch) + SB(14 + ch);
      o[3 + ch] = SB(8 + ch) + 4 * SB(11 + ch) + 6 * SB(14 + ch) + 4 * SB(17 + ch) + SB(20 + ch);
    }
#undef SB
  };
  int H[5][6];                                            // ring: source rows 2y - 2 .. 2y + 2 of the current output row
  hrow(2 * y0 - 2, H[0]);
  hrow(2 * y0 - 1, H[1]);
  hrow(2 * y0, H[2]);
#pragma unroll
  for (int k = 0; k < PD_ROWS; ++k) {
    const int y = y0 + k;
    if (y < dh) {                                          // wave-uniform
      // slots (2k + j) % 5 hold source row 2y - 2 + j
      hrow(2 * y + 1, H[(2 * k + 3) % 5]);
      hrow(2 * y + 2, H[(2 * k + 4) % 5]);
      uint32_t v[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const int acc = H[(2 * k) % 5][c] + 4 * H[(2 * k + 1) % 5][c] + 6 * H[(2 * k + 2) % 5][c] + 4 * H[(2 * k + 3) % 5][c] +
                        H[(2 * k + 4) % 5][c];
        v[c] = (uint32_t)((acc + 128) >> 8);
      }
      uint16_t *o = (uint16_t *)(dst + ((size_t)y * dw + 2 * xp) * 3);         // 6 bytes at an even offset
      o[0] = (uint16_t)(v[0] | (v[1] << 8));
      o[1] = (uint16_t)(v[2] | (v[3] << 8));
      o[2] = (uint16_t)(v[4] | (v[5] << 8));
    }
  }
}

int fl_launch_pyrdown_bgr(fl_context *ctx, const uint8_t *src, size_t in_stride, uint8_t *dst, size_t out_stride,
                          int n_frames, int w, int h)
{
  const int dw = w / 2, dh = h / 2;
  // the pair kernel stores 16-bit words: rows and frames of the output must start at even addresses; its last pair
  // reflects at an even w (an odd w has one more source column: the general kernel)
  const bool pairs_ok = dw >= 8 && (w & 1) == 0 && (dw & 1) == 0 && ((3 * dw) & 1) == 0 && (out_stride & 1) == 0 && (((size_t)dst) & 1) == 0;
  if (!pairs_ok) {
    dim3 grid((dw + 31) / 32, (dh + 7) / 8, n_frames);
    hipLaunchKernelGGL(k_pyrdown_general, grid, dim3(256), 0, ctx->stream, src, in_stride, dst, out_stride, w, h);
  } else {
    dim3 grid((dw / 2 + 63) / 64, (dh + 4 * PD_ROWS - 1) / (4 * PD_ROWS), n_frames);
    hipLaunchKernelGGL(k_pyrdown_pairs, grid, dim3(256), 0, ctx->stream, src, in_stride, dst, out_stride, w, h);
  }
  FL_HIP(ctx, hipGetLastError());
  return FL_OK;
}

// ------------------------------------------------------------------------------------------
// NORMAL_LUT[20][20][20] (linemod/normal_lut.i): independent of its first index; entry [y][x]
// is 1 << k with k the first of the 8 directions k*45deg maximising (x-10)cos + (y-10)sin.
// The 400 distinct bytes are generated on the host by the same rule as oracle/frontend_oracle.c
// and uploaded once.
__constant__ uint8_t c_normal_lut[400];
static bool g_normal_lut_ready[64] = {false};

static int ensure_normal_lut(fl_context *ctx)
{
  if (ctx->device < 64 && g_normal_lut_ready[ctx->device]) return FL_OK;
  uint8_t lut[400];
  for (int y = 0; y < 20; ++y)
    for (int x = 0; x < 20; ++x) {
      double best = -1e300;
      int bk = 0;
      for (int k = 0; k < 8; ++k) {
        double a = k * (3.14159265358979323846 / 4);
        double d = (x - 10) * cos(a) + (y - 10) * sin(a);
        if (d > best + 1e-9) { best = d; bk = k; }
      }
      lut[y * 20 + x] = (uint8_t)(1 << bk);
    }
  FL_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(c_normal_lut), lut, sizeof(lut)));
  if (ctx->device < 64) g_normal_lut_ready[ctx->device] = true;
  return FL_OK;
}

// accumBilateral (linemod.cpp:567-579) over the 8 ring neighbours, restated on what it adds up to.  With
// f_k = |delta_k| < threshold and offsets (i, j) in {-5, 0, 5}:  A[0] = sum f*i*i = 25 * #{f_k : i != 0},
// A[3] likewise for j, A[1] = sum f*i*j = 25 * (f(-,-) + f(+,+) - f(+,-) - f(-,+)), b[0] = sum f*i*delta =
// 5 * (sum over i = +5 of f*delta  -  sum over i = -5), b[1] likewise for j.  The same integers as the reference's
// `long` accumulation (|A| <= 150, |b| <= 30 * (threshold - 1)), in 32-bit registers.
//
// k_depth_quantize: quantizedNormals (linemod.cpp:595-683) fused with the medianBlur(5) that ends
// it (:684).  Same execution shape as k_color_quantize: a wavefront owns 64 adjacent columns (60
// outputs + 2 halo columns per side), walks chunk_rows output rows (fl_eager_chunk_rows: the first output row of a chunk
// costs four more rows of normals) and keeps the last five rows of patterns in registers.
// The depth taps come from a register ring: a lane holds the depth at its columns x - 5, x, x + 5 for the rows c - 5 .. c + 5
// of its current row c (33 registers), so a step loads one row at three columns instead of three rows at three columns, and
// the ring's slots trade roles over a loop body of eleven steps (k_color_quantize's seven-row ring does the same).  Strip,
// chunk, rows and the row addresses of depth, dst and dst1 are scalar and advance by scalar additions; loads and stores take
// a scalar base and a 32-bit lane offset.  Measured (profiles/README.md): 5.63 -> 4.98 ms per 4096 VGA frames, most of it
// from the scalar addresses; the row-ahead and packed rings were slower than this one.
// The codes are 0 or one-hot, i.e. 9 classes ordered like their byte values, and the exact 5x5 median is
// the first class whose CUMULATIVE count reaches 13.  A pixel of class c therefore contributes the
// pattern "1 in every 4-bit field i >= c" (fields 0..7; class 8's own field would always hold 25 and is
// implied): five rows add up to a column word (fields <= 5), the x-1, x+1 / x-2, x+2 columns come by
// whole-wave DPP shifts, 3 + 2 columns are added in 4-bit fields (<= 15, <= 10), and the ">= 13" test runs on
// the even / odd fields widened to bytes (sum + 115 sets bit 7).  The flags are monotone in the class, so
// median class = 8 - popcount.  The un-medianed normal image never exists in memory.
// dst1 (null: none) is the next pyramid level's image, cv::resize INTER_NEAREST to half size, for even w and h: the lane
// that stores pixel (yo, x) with both even stores the same byte to dst1(yo / 2, x / 2) -- a separate pass would read the
// whole level-0 image back for it.
#define DQ_COLS 60

__device__ __forceinline__ unsigned dq_pattern(unsigned cls) { return cls >= 8u ? 0u : 0x11111111u << (4u * cls); }

// a * b of factors that fit 24 bits (signed: -2^23 .. 2^23 - 1; unsigned: below 2^24), low 32 bits of the product: the
// full-rate v_mul_i32_i24 / v_mul_u32_u24, whatever the compiler can or cannot prove about the factors (dq_normal_pattern)
__device__ __forceinline__ int dq_mul_i24(int a, int b)
{
  int r;
  asm("v_mul_i32_i24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ unsigned dq_mul_u24(unsigned a, unsigned b)
{
  unsigned r;
  asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// K * b, K a constant of the instruction (no register holds it)
template <int K>
__device__ __forceinline__ int dq_mul_i24_by(int b)
{
  int r;
  asm("v_mul_i32_i24 %0, %1, %2" : "=v"(r) : "n"(K), "v"(b));
  return r;
}
// K * b + c, K an inline constant of the instruction (0 .. 64): v_mad_u32_u24
template <unsigned K>
__device__ __forceinline__ unsigned dq_mad_u24_by(unsigned b, unsigned c)
{
  static_assert(K <= 64, "not an inline constant");
  unsigned r;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(b), "n"(K), "v"(c));
  return r;
}

// The normal of one pixel from values: its depth d and the eight ring neighbours n0..n7, in the order (-,-) (0,-) (+,-) (-,0)
// (+,0) (-,+) (0,+) (+,+).  interior: y >= 5 && y < h - 6 && x >= 5 && x < w - 6 (loop bounds :619, :624); of a lane that is not
// interior, or whose d is not below distance_threshold, nothing is looked at (its taps are clamped into the image and mean
// nothing).
__device__ __forceinline__ unsigned dq_normal_pattern(bool interior, int d, int n0, int n1, int n2, int n3, int n4, int n5, int n6,
                                                      int n7, int distance_threshold, int difference_threshold, const uint8_t *lut)
{
  if (!interior) return dq_pattern(0);
  if (!(d < distance_threshold)) return dq_pattern(0);
  const int t = difference_threshold;
  const unsigned span = t > 0 ? (unsigned)(2 * t - 1) : 0u;   // t <= 0 admits nothing
  // |e| < t  <=>  (unsigned)(e + t - 1) < 2t - 1, e = n - d: u = n - (d - (t - 1)) is that left side                :569
  const unsigned tm1 = (unsigned)t - 1u, lo = (unsigned)d - tm1;
  const unsigned u0 = (unsigned)n0 - lo, u1 = (unsigned)n1 - lo, u2 = (unsigned)n2 - lo, u3 = (unsigned)n3 - lo,
                 u4 = (unsigned)n4 - lo, u5 = (unsigned)n5 - lo, u6 = (unsigned)n6 - lo, u7 = (unsigned)n7 - lo;
  float nx, ny, nz;
  // Decided once per wave-step (one ballot over the lanes still here, of the largest of the eight u against the span): does
  // every lane that got this far admit all eight neighbours?  Then for each of them f_k = 1 and m_k = e_k, so A0 = A3 = 150,
  // A1 = 0, det = 22500, the three d on each side of b0 and b1 cancel, ddx = 150 * b0, ddy = 150 * b1, and the same integers
  // come from the neighbours alone: nx = 617 * 150 * 5 * ((n2 + n4 + n7) - (n0 + n3 + n5)), ny likewise, nz = -22500 * d.
  // With t <= 400 the bracket is at most 6 * 399, the factor 462750 fits 24 bits and the products 31 (22500 * 65535 < 2^31).
  // Smooth surfaces are the common case.  Everything only the general path needs -- the differences e_k, the
  // eight compares, the selects, the counts, A, det and their products -- stays behind this wave-uniform branch (eight masks
  // ANDed on the scalar unit instead of the maximum kept sixteen more scalar and four more vector registers alive across it).
  const unsigned umax = max(max(max(u0, u1), max(u2, u3)), max(max(u4, u5), max(u6, u7)));
  if (t <= 400 && __builtin_amdgcn_ballot_w64(umax >= span) == 0) {
    nx = (float)dq_mul_i24_by<462750>((n2 + n4 + n7) - (n0 + n3 + n5));
    ny = (float)dq_mul_i24_by<462750>((n5 + n6 + n7) - (n0 + n1 + n2));
    nz = (float)dq_mul_i24_by<-22500>(d);
  } else {
    const int e0 = (int)(u0 - tm1), e1 = (int)(u1 - tm1), e2 = (int)(u2 - tm1), e3 = (int)(u3 - tm1), e4 = (int)(u4 - tm1),
              e5 = (int)(u5 - tm1), e6 = (int)(u6 - tm1), e7 = (int)(u7 - tm1);
    const bool g0 = u0 < span, g1 = u1 < span, g2 = u2 < span, g3 = u3 < span, g4 = u4 < span, g5 = u5 < span, g6 = u6 < span,
               g7 = u7 < span;
    const int f0 = g0, f1 = g1, f2 = g2, f3 = g3, f4 = g4, f5 = g5, f6 = g6, f7 = g7;
    const int m0 = g0 ? e0 : 0, m1 = g1 ? e1 : 0, m2 = g2 ? e2 : 0, m3 = g3 ? e3 : 0, m4 = g4 ? e4 : 0, m5 = g5 ? e5 : 0,
              m6 = g6 ? e6 : 0, m7 = g7 ? e7 : 0;
    const int corners = f0 + f2 + f5 + f7;
    // Every factor below fits 24 bits: |A| <= 150, 0 <= det <= 22500, and with t <= 400 |b| <= 30 * 399, |dd| < 3.0e6, d < 65536.
    // The products of det and of the t <= 400 path are the full-rate 24-bit multiplies BY NAME (dq_mul_i24, dq_mul_u24).  __mul24 is a
    // 32-bit multiply of the arguments' sign-extended low 24 bits, and what the compiler makes of it depends on what it knows
    // of them: it folded the extension into a factor that was itself a product (5 * x became (x * (5 << 8)) >> 8) and, with d's
    // 16 bits known, dropped it from det * d, and each time a v_mul_lo_u32 (quarter rate) was left.  The products by 5 and
    // by 25 are plain C: v_lshl_add_u32, and 24-bit multiplies by the constant.
    const int A0 = 25 * (corners + f3 + f4), A3 = 25 * (corners + f1 + f6), A1 = 25 * ((f0 + f7) - (f2 + f5));
    const int det = (int)dq_mul_u24((unsigned)A0, (unsigned)A3) - dq_mul_i24(A1, A1);       // 0 <= det <= 22500: |A1| <= 25 * corners <= A0, A3
    const int b0 = 5 * ((m2 + m4 + m7) - (m0 + m3 + m5)), b1 = 5 * ((m5 + m6 + m7) - (m0 + m1 + m2));
    if (t <= 400) {
      // |b| <= 30 * 399, |dd| <= 250 * |b| < 3.0e6: 617 * dd and det * d (<= 22500 * 65535) fit in int32
      const int ddx = dq_mul_i24(A3, b0) - dq_mul_i24(A1, b1), ddy = dq_mul_i24(A0, b1) - dq_mul_i24(A1, b0);
      nx = (float)dq_mul_i24_by<617>(ddx);
      ny = (float)dq_mul_i24_by<617>(ddy);
      nz = (float)(-(int)dq_mul_u24((unsigned)det, (unsigned)d));
    } else {
      const long long ddx = (long long)A3 * b0 - (long long)A1 * b1, ddy = -(long long)A1 * b0 + (long long)A0 * b1;
      nx = (float)(617LL * ddx);
      ny = (float)(617LL * ddy);
      nz = (float)(-(long long)det * d);
    }
  }
  // nx, ny, nz are integers (converted, beyond 2^24 rounded, to float): their sum of squares is 0 or in [1, 2^80) -- 617 * dd
  // stays below 2^39 at any threshold, det * d below 2^31 -- and its root s is 0 exactly where the sum is, else in [1, 2^40):
  // inside the domains of sqrt_rn and rcp_rn (fl_ranged_math.h), which give the bits of sqrtf(sum) and 1.0f / s
  const float sum = nx * nx + ny * ny + nz * nz;
  if (!(sum > 0)) return dq_pattern(0);                     // s == 0: shadows of the depth sensor
  const float s = sqrt_rn(sum);
  // (Round 4 measured the LUT indices from a v_rsq_f32 ESTIMATE with the correctly rounded sqrtf + division only for lanes
  // within 4e-5 of a bin edge -- exact by construction, bit-equal in the tests -- and it was 2 % SLOWER (front-end 18.04
  // against 17.70 ms per 4096 eager frames): the test for "near an edge" costs what the two correctly rounded operations
  // cost, and a wavefront takes the exact branch whenever one of its 64 lanes is near an edge.  profiles/README.md.)
  const float inv = rcp_rn(s);
  nx *= inv;
  ny *= inv;
  nz *= inv;
  const int v1 = (int)(nx * 10 + 10);
  const int v2 = (int)(ny * 10 + 10);
  const int v3 = (int)(nz * 20 + 20);
  // Q7: v3 == 20 is an out-of-bounds read in the reference; defined as 0 here
  if (!(v1 >= 0 && v1 <= 19 && v2 >= 0 && v2 <= 19 && v3 >= 0 && v3 <= 19)) return dq_pattern(0);
  // index < 400: one v_mad_u32_u24 (as v2 * 20 + v1 the compiler widens it to a v_mad_u64_u32, quarter rate)
  const unsigned v = lut[dq_mad_u24_by<20>((unsigned)v2, (unsigned)v1)];
  return dq_pattern(v ? (unsigned)(32 - __clz(v)) : 0u);   // 0 -> class 0, 1<<k -> class k+1 (ascending in value)
}

#define DQ_RING 11                                         // depth rows c - 5 .. c + 5 of the current row of normals c

__global__ __launch_bounds__(256) void k_depth_quantize(const uint16_t *__restrict__ depth_, size_t in_stride,
                                                        uint8_t *__restrict__ dst_, size_t out_stride, int w, int h,
                                                        int distance_threshold, int difference_threshold, int nstrips,
                                                        int nchunks, int chunk_rows, uint8_t *__restrict__ dst1_,
                                                        size_t out1_stride)
{
  __shared__ uint8_t s_lut[400];                           // NORMAL_LUT's 20x20 face: a per-lane lookup every row
  for (int k = threadIdx.x; k < 400; k += 256) s_lut[k] = c_normal_lut[k];
  __syncthreads();
  // the wave index is the same in all 64 lanes: as a scalar it keeps the strip, the rows and the row addresses on the scalar unit
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + wave;
  if (item >= nstrips * nchunks) return;
  const int strip = item % nstrips, chunk = item / nstrips;
  const uint16_t *depth = depth_ + (size_t)blockIdx.z * in_stride;
  uint8_t *dst = dst_ + (size_t)blockIdx.z * out_stride;
  uint8_t *dst1 = dst1_ ? dst1_ + (size_t)blockIdx.z * out1_stride : nullptr;
  const int x = strip * DQ_COLS + lane - 2;
  const int xc = clampi(x, 0, w - 1);                      // medianBlur replicates the border
  const int y0 = chunk * chunk_rows, y1 = min(h, y0 + chunk_rows);
  // The lane's 32-bit byte offsets from a row's scalar address: the three tap columns, clamped into the row (a clamped one
  // belongs to a pixel that is not interior), and its pixel in dst and dst1.  lane_off's empty asm keeps an offset a 32-bit value
  // where it is used: widened to 64 bits once, ahead of the loop, it turns every access into a 64-bit vector addition
  // instead of the instruction's scalar-base form.
  unsigned ol = 2u * (unsigned)max(xc - 5, 0), oc = 2u * (unsigned)xc, orr = 2u * (unsigned)min(xc + 5, w - 1);
  unsigned ox = (unsigned)x, ox1 = (unsigned)x >> 1;
  auto lane_off = [](unsigned &off) __attribute__((always_inline)) { asm volatile("" : "+v"(off)); return off; };
  auto tap = [&](const char *rowp, unsigned &off) __attribute__((always_inline)) { return (int)*(const uint16_t *)(rowp + lane_off(off)); };
  const bool xin = xc >= 5 && xc < w - 6;
  const bool writes = lane >= 2 && lane < 2 + DQ_COLS && x < w;
  const int cs = max(y0 - 2, 0), ce = min(y1 + 1, h - 1);  // the rows of normals this chunk's medians take
  const size_t row_bytes = 2 * (size_t)w;
  int RL[DQ_RING], RC[DQ_RING], RR[DQ_RING];               // columns xc - 5, xc, xc + 5; in step P row c + j is in slot (P + 5 + j) % DQ_RING
  // prologue: rows cs - 5 .. cs + 4, clamped into the image, into slots 0 .. 9
#pragma unroll
  for (int i = 0; i < DQ_RING - 1; ++i) {
    const char *rowp = (const char *)depth + (size_t)clampi(cs + i - 5, 0, h - 1) * row_bytes;
    RL[i] = tap(rowp, ol);
    RC[i] = tap(rowp, oc);
    RR[i] = tap(rowp, orr);
  }
  const char *ldp = (const char *)depth + (size_t)min(cs + 5, h - 1) * row_bytes;    // the row the first step loads
  uint8_t *orow = dst + (size_t)y0 * (size_t)w;            // the output rows' addresses: scalar, advanced by additions
  uint8_t *orow1 = dst1 ? dst1 + (size_t)(y0 >> 1) * (size_t)(w >> 1) : nullptr;
  unsigned p0 = 0, p1 = 0, p2 = 0, p3 = 0, p4 = 0;         // cumulative-count patterns of the last five rows, p0 newest
  auto push = [&](unsigned pat) __attribute__((always_inline)) { p4 = p3; p3 = p2; p2 = p1; p1 = p0; p0 = pat; };
  // the median and the stores at row yo = yv - 2
  auto finish = [&](int yv) __attribute__((always_inline)) {
    if (yv < y0 + 2) return;                               // wave-uniform
    const unsigned col = p0 + p1 + p2 + p3 + p4;           // fields <= 5
    // single DPP moves that leave 0 where a shift has no source lane: a1 of lane 63, a2 of lanes 62 and 63, b1 of lane 0, b2 of
    // lanes 0 and 1.  The lanes that store are 2 .. 61: lane 61 takes col of lanes 59 .. 63, lane 2 of lanes 0 .. 4
    const unsigned a1 = wave_from_next0(col), b1 = wave_from_prev0(col), a2 = wave_from_next0(a1), b2 = wave_from_prev0(b1);
    const unsigned s3 = col + a1 + b1, s2 = a2 + b2;       // fields <= 15, <= 10
    const unsigned te = (s3 & 0x0F0F0F0Fu) + (s2 & 0x0F0F0F0Fu) + 0x73737373u;
    const unsigned to = ((s3 >> 4) & 0x0F0F0F0Fu) + ((s2 >> 4) & 0x0F0F0F0Fu) + 0x73737373u;
    const int idx = 8 - __popc((te & 0x80808080u) | ((to & 0x80808080u) >> 1));
    const int yo = yv - 2;
    if (writes) {
      const uint8_t v = idx ? (uint8_t)(1u << (idx - 1)) : 0;
      orow[lane_off(ox)] = v;
      if (orow1 && !((yo | x) & 1)) orow1[lane_off(ox1)] = v;
    }
    orow += w;
    if (orow1 && (yo & 1)) orow1 += w >> 1;
  };
  // Virtual rows y0 - 2 .. y1 + 1.  Rows < 0 and >= h repeat rows 0 and h - 1, which are never interior: they push
  // dq_pattern(0) and leave the depth ring alone.  Rows cs .. ce take one step each: step P of the unrolled body loads row c + 5
  // (clamped) into slot P + 10, which row c - 6 has left, and computes with slots P, P + 5, P + 10 (rows c - 5, c, c + 5), so
  // no slot is moved.
  int yv = y0 - 2;
  for (; yv < 0; ++yv) push(dq_pattern(0));                // nothing follows: yv < y0 + 2
  auto step = [&](auto phase) __attribute__((always_inline)) {
    constexpr int P = decltype(phase)::value, A = P % DQ_RING, C = (P + 5) % DQ_RING, B = (P + 10) % DQ_RING;
    RL[B] = tap(ldp, ol);
    RC[B] = tap(ldp, oc);
    RR[B] = tap(ldp, orr);
    if (yv + 5 < h - 1) ldp += row_bytes;                  // scalar
    push(dq_normal_pattern(xin && yv >= 5 && yv < h - 6, RC[C], RL[A], RC[A], RR[A], RL[C], RR[C], RL[B], RC[B], RR[B],
                           distance_threshold, difference_threshold, s_lut));
    finish(yv);
    ++yv;
  };
#define DQ_STEP(P)                                                                                                                  \
  if (yv > ce) break;                                                                                                               \
  step(std::integral_constant<int, P>());
  for (;;) {
    DQ_STEP(0) DQ_STEP(1) DQ_STEP(2) DQ_STEP(3) DQ_STEP(4) DQ_STEP(5) DQ_STEP(6) DQ_STEP(7) DQ_STEP(8) DQ_STEP(9) DQ_STEP(10)
  }
#undef DQ_STEP
  for (; yv <= y1 + 1; ++yv) {
    push(dq_pattern(0));
    finish(yv);
  }
}

int fl_launch_quantized_normals(fl_context *ctx, const uint16_t *depth, size_t in_stride, uint8_t *dst,
                                size_t out_stride, uint8_t *dst1, size_t out1_stride, int n_frames, int w, int h,
                                int distance_threshold, int difference_threshold)
{
  static long per_cu = 0;
  int rc = ensure_normal_lut(ctx);
  if (rc) return rc;
  if (dst1 && ((w | h) & 1)) return fl_set_error(ctx, FL_ERR_INVALID, "fused half-size normals need even sizes, got %dx%d", w, h);
  const int nstrips = (w + DQ_COLS - 1) / DQ_COLS;
  const int rows = fl_eager_chunk_rows(ctx, waves_per_cu(k_depth_quantize, &per_cu), nstrips, n_frames, h);
  const int nchunks = (h + rows - 1) / rows;
  dim3 grid((nstrips * nchunks + 3) / 4, 1, n_frames);
  hipLaunchKernelGGL(k_depth_quantize, grid, dim3(256), 0, ctx->stream, depth, in_stride / sizeof(uint16_t), dst, out_stride,
                     w, h, distance_threshold, difference_threshold, nstrips, nchunks, rows, dst1, out1_stride);
  FL_HIP(ctx, hipGetLastError());
  return FL_OK;
}

// cv::resize INTER_NEAREST to half size (linemod.cpp:731): sx = min(floor(x * (1 / (dw / w))), w - 1).  For even w and h
// that is src(2y, 2x); then one thread makes 4 output pixels from one aligned 8-byte load and stores one dword (the
// one-pixel-per-thread version spent its time on byte loads and byte stores).  Other sizes take the general kernel.
__global__ __launch_bounds__(256) void k_resize_nn_half4(const uint8_t *__restrict__ src_, size_t in_stride,
                                                         uint8_t *__restrict__ dst_, size_t out_stride, int w, int h)
{
  const int dw = w / 2, dh = h / 2;
  const int x4 = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (4 * x4 >= dw || y >= dh) return;
  const uint8_t *src = src_ + (size_t)blockIdx.z * in_stride;
  uint8_t *dst = dst_ + (size_t)blockIdx.z * out_stride;
  uint2 v;
  __builtin_memcpy(&v, __builtin_assume_aligned(src + (size_t)(2 * y) * w + 8 * x4, 8), 8);
  const uint32_t o = (v.x & 0xFFu) | ((v.x >> 8) & 0xFF00u) | ((v.y & 0xFFu) << 16) | ((v.y << 8) & 0xFF000000u);
  *(uint32_t *)(dst + (size_t)y * dw + 4 * x4) = o;
}

__global__ __launch_bounds__(256) void k_resize_nn_half(const uint8_t *__restrict__ src_, size_t in_stride,
                                                        uint8_t *__restrict__ dst_, size_t out_stride, int w, int h)
{
  const int dw = w / 2, dh = h / 2;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  const uint8_t *src = src_ + (size_t)blockIdx.z * in_stride;
  uint8_t *dst = dst_ + (size_t)blockIdx.z * out_stride;
  int sx = (int)floor(x * (1.0 / ((double)dw / w))), sy = (int)floor(y * (1.0 / ((double)dh / h)));
  sx = min(sx, w - 1);
  sy = min(sy, h - 1);
  dst[(size_t)y * dw + x] = src[(size_t)sy * w + sx];
}

// even sizes: 1 / ((w/2) / w) == 2 exactly, so the source pixel is (2y, 2x); w % 8 == 0 keeps the 8-byte loads aligned
static bool resize_nn_half_fast(const uint8_t *src, size_t in_stride, const uint8_t *dst, size_t out_stride, int w, int h)
{
  return (w % 8) == 0 && (h % 2) == 0 && ((in_stride | out_stride) & 7) == 0 && ((((size_t)src) | ((size_t)dst)) & 7) == 0;
}

int fl_launch_resize_nn_half(fl_context *ctx, const uint8_t *src, size_t in_stride, uint8_t *dst, size_t out_stride,
                             int n_frames, int w, int h)
{
  if (resize_nn_half_fast(src, in_stride, dst, out_stride, w, h)) {
    dim3 grid((w / 8 + 63) / 64, (h / 2 + 3) / 4, n_frames);
    hipLaunchKernelGGL(k_resize_nn_half4, grid, dim3(256), 0, ctx->stream, src, in_stride, dst, out_stride, w, h);
  } else {
    dim3 grid((w / 2 + 63) / 64, (h / 2 + 3) / 4, n_frames);
    hipLaunchKernelGGL(k_resize_nn_half, grid, dim3(256), 0, ctx->stream, src, in_stride, dst, out_stride, w, h);
  }
  FL_HIP(ctx, hipGetLastError());
  return FL_OK;
}

// ------------------------------------------------------------------------------------------
// Modality::process + pyrDown + quantize for every level (linemod.cpp:1369-1416) of n_frames frames.  Default modality
// parameters (linemod.cpp:515-519, 827-832).  The images of level l are frame-strided arrays: the colour image (level 0: the
// input), the quantised colour image and, with a depth modality, the quantised normals.  Level 1's normals come out of the
// depth quantiser itself where the half-size rule is src(2y, 2x) (the sizes resize_nn_half_fast takes); deeper levels and other
// sizes take k_resize_nn_half*.  first_color_level: colour levels below it are left to the lazy path.
struct FlFrontImages {
  int L, M;
  int w[FL_MAX_LEVELS], h[FL_MAX_LEVELS];
  uint8_t *bgr[FL_MAX_LEVELS], *qcolor[FL_MAX_LEVELS], *qdepth[FL_MAX_LEVELS];
  size_t stride;
};
static int launch_front_images(fl_context *ctx, const FlFrontImages &im, int n_frames, const uint8_t *bgr, size_t bgr_stride,
                               const uint16_t *depth, size_t depth_stride, int first_color_level)
{
  int rc;
  bool fused1 = false;
  for (int l = 0; l < im.L; ++l) {
    if (l > 0) {
      rc = fl_launch_pyrdown_bgr(ctx, l == 1 ? bgr : im.bgr[l - 1], l == 1 ? bgr_stride : im.stride, im.bgr[l], im.stride, n_frames,
                                 im.w[l - 1], im.h[l - 1]);
      if (rc) return rc;
      if (im.M > 1 && !(l == 1 && fused1)) {
        rc = fl_launch_resize_nn_half(ctx, im.qdepth[l - 1], im.stride, im.qdepth[l], im.stride, n_frames, im.w[l - 1], im.h[l - 1]);
        if (rc) return rc;
      }
    } else if (im.M > 1) {
      fused1 = im.L > 1 && resize_nn_half_fast(im.qdepth[0], im.stride, im.qdepth[1], im.stride, im.w[0], im.h[0]);
      rc = fl_launch_quantized_normals(ctx, depth, depth_stride, im.qdepth[0], im.stride, fused1 ? im.qdepth[1] : nullptr, im.stride,
                                       n_frames, im.w[0], im.h[0], 2000, 50);
      if (rc) return rc;
    }
    if (l < first_color_level) continue;
    rc = fl_launch_quantized_orientations(ctx, l == 0 ? bgr : im.bgr[l], l == 0 ? bgr_stride : im.stride, im.qcolor[l], im.stride,
                                          n_frames, im.w[l], im.h[l], 10.0f);
    if (rc) return rc;
  }
  return FL_OK;
}

int fl_launch_frontend(fl_detector *det, int n_frames, const uint8_t *bgr, size_t bgr_stride, const uint16_t *depth,
                       size_t depth_stride, bool allow_lazy)
{
  fl_context *ctx = det->ctx;
  // Lazy fine levels: everything that feeds the coarsest level (colour pyramid, depth quantisation and its NN
  // pyramid, the coarsest colour quantisation) runs here; the colour quantisation of the finer levels waits for the
  // scan's candidates (fl_launch_lazy_level).
  det->lazy = allow_lazy && det->lazy_capable && !det->eager_env;
  det->lazy_bgr = bgr;
  det->lazy_bgr_stride = bgr_stride;
  FlFrontImages im;
  im.L = det->L;
  im.M = det->M;
  im.stride = det->ws_stride;
  for (int l = 0; l < det->L; ++l) {
    const FlLevelGeom &g = det->geom[l];
    im.w[l] = g.w;
    im.h[l] = g.h;
    im.bgr[l] = det->d_ws + g.bgr_off;
    im.qcolor[l] = det->d_ws + g.quant_off[0];
    im.qdepth[l] = det->d_ws + g.quant_off[1];
  }
  int rc = launch_front_images(ctx, im, n_frames, bgr, bgr_stride, depth, depth_stride, det->lazy ? det->L - 1 : 0);
  if (rc) return rc;
  if (det->have_times) FL_HIP(ctx, hipEventRecord(det->ev[1], ctx->stream));
  return FL_OK;
}

// Development / test aid (not part of the ABI): launch_front_images -- the launches fl_launch_frontend queues for an eager
// batch with both modalities -- on n_frames host frames of ANY size, also those no detector can be finalized for (LINEMOD's
// own asserts on T and rows * cols do not concern the front-end).  out: per frame, level after level, the quantised colour
// image, the quantised normals and (level >= 1) the colour image, (5 or 2) * w_l * h_l bytes per level with w_l = w >> l.
extern "C" int fl_dev_front_images(fl_context *ctx, const uint8_t *bgr, const uint16_t *depth, int n_frames, int w, int h, int levels,
                                   uint8_t *out, size_t out_bytes)
{
  if (!ctx || !bgr || !depth || !out || n_frames < 1 || levels < 1 || levels > FL_MAX_LEVELS || w < 3 || h < 3 || (w >> (levels - 1)) < 3 ||
      (h >> (levels - 1)) < 3)
    return FL_ERR_INVALID;
  FL_HIP(ctx, hipSetDevice(ctx->device));
  FlFrontImages im;
  im.L = levels;
  im.M = 2;
  size_t off = 0;
  for (int l = 0; l < levels; ++l) {
    im.w[l] = w >> l;
    im.h[l] = h >> l;
    const size_t px = (size_t)im.w[l] * im.h[l];
    im.qcolor[l] = (uint8_t *)off;
    im.qdepth[l] = (uint8_t *)(off + fl_align(px, 256));
    im.bgr[l] = (uint8_t *)(off + 2 * fl_align(px, 256));
    off += 2 * fl_align(px, 256) + (l ? fl_align(3 * px, 256) : 0);
  }
  const size_t packed = off, fb = (size_t)w * h * 3, fd = (size_t)w * h * 2, in_b = fl_align(fb * n_frames, 256);
  size_t need = 0;
  for (int l = 0; l < levels; ++l) need += (size_t)im.w[l] * im.h[l] * (l ? 5 : 2);
  if (out_bytes < need * n_frames) return fl_set_error(ctx, FL_ERR_INVALID, "fl_dev_front_images: out holds %zu bytes, %zu needed", out_bytes, need * n_frames);
  void *s = nullptr;
  int rc = fl_scratch(ctx, in_b + fl_align(fd * n_frames, 256) + packed * n_frames, &s);
  if (rc) return rc;
  uint8_t *d_bgr = (uint8_t *)s, *d_depth = d_bgr + in_b, *d_im = d_depth + fl_align(fd * n_frames, 256);
  im.stride = packed;
  for (int l = 0; l < levels; ++l) {
    im.qcolor[l] = d_im + (size_t)im.qcolor[l];
    im.qdepth[l] = d_im + (size_t)im.qdepth[l];
    im.bgr[l] = d_im + (size_t)im.bgr[l];
  }
  FL_HIP(ctx, hipMemcpyAsync(d_bgr, bgr, fb * n_frames, hipMemcpyHostToDevice, ctx->stream));
  FL_HIP(ctx, hipMemcpyAsync(d_depth, depth, fd * n_frames, hipMemcpyHostToDevice, ctx->stream));
  FL_HIP(ctx, hipMemsetAsync(d_im, 0xFF, packed * n_frames, ctx->stream));      // never a quantised byte: an unwritten pixel shows
  if ((rc = launch_front_images(ctx, im, n_frames, d_bgr, fb, (const uint16_t *)d_depth, fd, 0))) return rc;
  for (int f = 0; f < n_frames; ++f)
    for (int l = 0; l < levels; ++l) {
      const size_t px = (size_t)im.w[l] * im.h[l];
      FL_HIP(ctx, hipMemcpyAsync(out, im.qcolor[l] + f * packed, px, hipMemcpyDeviceToHost, ctx->stream));
      FL_HIP(ctx, hipMemcpyAsync(out + px, im.qdepth[l] + f * packed, px, hipMemcpyDeviceToHost, ctx->stream));
      if (l) FL_HIP(ctx, hipMemcpyAsync(out + 2 * px, im.bgr[l] + f * packed, 3 * px, hipMemcpyDeviceToHost, ctx->stream));
      out += (l ? 5 : 2) * px;
    }
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FL_OK;
}

// Development / test aid (not part of the ABI): fl_launch_quantized_orientations_mag -- k_color_quantize<true, *>, the
// instantiations template extraction launches -- on n_frames packed host frames of w x h.  quantized: n_frames * w * h
// labels; magnitude: n_frames * w * h squared gradient magnitudes.  Both are uploaded as given and read back, so what the
// kernel does not write returns unchanged.
extern "C" int fl_dev_quantized_orientations_mag(fl_context *ctx, const uint8_t *bgr, int n_frames, int w, int h, float weak_threshold,
                                                 uint8_t *quantized, float *magnitude)
{
  if (!ctx || !bgr || !quantized || !magnitude || n_frames < 1 || w < 3 || h < 3) return FL_ERR_INVALID;
  FL_HIP(ctx, hipSetDevice(ctx->device));
  const size_t px = (size_t)w * h, in_b = fl_align(px * 3 * n_frames, 256), q_b = fl_align(px * n_frames, 256);
  void *s = nullptr;
  int rc = fl_scratch(ctx, in_b + q_b + px * 4 * n_frames, &s);
  if (rc) return rc;
  uint8_t *d_bgr = (uint8_t *)s, *d_q = d_bgr + in_b;
  float *d_mag = (float *)(d_q + q_b);
  FL_HIP(ctx, hipMemcpyAsync(d_bgr, bgr, px * 3 * n_frames, hipMemcpyHostToDevice, ctx->stream));
  FL_HIP(ctx, hipMemcpyAsync(d_q, quantized, px * n_frames, hipMemcpyHostToDevice, ctx->stream));
  FL_HIP(ctx, hipMemcpyAsync(d_mag, magnitude, px * 4 * n_frames, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = fl_launch_quantized_orientations_mag(ctx, d_bgr, px * 3, d_q, px, n_frames, w, h, weak_threshold, d_mag))) return rc;
  FL_HIP(ctx, hipMemcpyAsync(quantized, d_q, px * n_frames, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipMemcpyAsync(magnitude, d_mag, px * 4 * n_frames, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FL_OK;
}

// Development / test aid (not part of the ABI): the functions of fl_ranged_math.h against the compiler's own operations, which
// this file's flags make correctly rounded, over EVERY argument first .. last of a domain (tests/test_gpu_ranged_math.py).
//   which 0: sqrt_rn(x) against sqrtf(x), 1: rcp_rn(x) against 1.0f / x, x the float with the bit pattern a;
//   which 2: div_rn(n, d) against n / d, n and d what fast_atan2_deg divides for |x| = a % 1021 and |y| = a / 1021 (both 0 .. 1020)
// Adds the number of results that differ in any bit to *n_bad and keeps the smallest such a in *first_bad.
#define FL_RM_SOBEL_MAX 1020u                              // |dx|, |dy| <= 4 * 255
__global__ __launch_bounds__(256) void k_ranged_math(int which, uint32_t first, uint32_t last, unsigned long long *n_bad, uint32_t *first_bad)
{
  const uint64_t count = (uint64_t)last - first + 1, stride = (uint64_t)gridDim.x * blockDim.x;
  unsigned bad = 0;
  uint32_t lowest = 0xFFFFFFFFu;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const uint32_t a = first + (uint32_t)i;
    float got, exp;
    if (which == 0) {
      const float x = __uint_as_float(a);
      got = sqrt_rn(x);
      exp = sqrtf(x);
    } else if (which == 1) {
      const float x = __uint_as_float(a);
      got = rcp_rn(x);
      exp = 1.0f / x;
    } else {
      const float ax = (float)(a % (FL_RM_SOBEL_MAX + 1u)), ay = (float)(a / (FL_RM_SOBEL_MAX + 1u));
      const bool steep = !(ax >= ay);
      const float n = steep ? ax : ay, d = (steep ? ay : ax) + (float)DBL_EPSILON;
      got = div_rn(n, d);
      exp = n / d;
    }
    if (__float_as_uint(got) != __float_as_uint(exp)) {
      ++bad;
      lowest = min(lowest, a);
    }
  }
  if (bad) {
    atomicAdd(n_bad, (unsigned long long)bad);
    atomicMin(first_bad, lowest);
  }
}

extern "C" int fl_dev_ranged_math(fl_context *ctx, int which, uint32_t first_bits, uint32_t last_bits, unsigned long long *n_mismatch,
                                  uint32_t *first_bad_bits)
{
  if (!ctx || !n_mismatch || !first_bad_bits || which < 0 || which > 2 || first_bits > last_bits ||
      (which == 2 && last_bits >= (FL_RM_SOBEL_MAX + 1u) * (FL_RM_SOBEL_MAX + 1u)))
    return FL_ERR_INVALID;
  FL_HIP(ctx, hipSetDevice(ctx->device));
  void *s = nullptr;
  int rc = fl_scratch(ctx, 16, &s);
  if (rc) return rc;
  unsigned long long *d_bad = (unsigned long long *)s;
  uint32_t *d_first = (uint32_t *)(d_bad + 1);
  FL_HIP(ctx, hipMemsetAsync(d_bad, 0, 8, ctx->stream));
  FL_HIP(ctx, hipMemsetAsync(d_first, 0xFF, 4, ctx->stream));
  hipLaunchKernelGGL(k_ranged_math, dim3(1024), dim3(256), 0, ctx->stream, which, first_bits, last_bits, d_bad, d_first);
  FL_HIP(ctx, hipGetLastError());
  FL_HIP(ctx, hipMemcpyAsync(n_mismatch, d_bad, 8, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipMemcpyAsync(first_bad_bits, d_first, 4, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FL_OK;
}

// Fine level `level` of a lazy batch, after k_mark_tiles: colour quantisation of the tiles in the "quantised pixels
// needed" bitmap, then both modalities' spread images in the rows/columns of the "spread bytes needed" bitmap.
int fl_launch_lazy_level(fl_detector *det, int n_frames, int level)
{
  fl_context *ctx = det->ctx;
  const FlLevelGeom &g = det->geom[level];
  const uint32_t *tiles = (const uint32_t *)(det->d_ws + det->off_tiles) + (size_t)level * FL_TILE_BLOCK_WORDS;
  const size_t tstride = det->ws_stride / sizeof(uint32_t);
  if (det->poison_env) {   // dev aid: a byte read outside the marked tiles must not look plausible
    FL_HIP(ctx, hipMemset2DAsync(det->d_ws + g.quant_off[0], det->ws_stride, 0xFF, (size_t)g.w * g.h, n_frames, ctx->stream));
    for (int m = 0; m < det->M; ++m)
      FL_HIP(ctx, hipMemset2DAsync(det->d_ws + g.spread_off[m], det->ws_stride, 0xFF, (size_t)g.w * g.h, n_frames, ctx->stream));
  }
  int rc = launch_color_quantize(ctx, level == 0 ? det->lazy_bgr : det->d_ws + g.bgr_off, level == 0 ? det->lazy_bgr_stride : det->ws_stride,
                                 det->d_ws + g.quant_off[0], det->ws_stride, n_frames, g.w, g.h, 10.0f, nullptr,
                                 tiles, tstride);
  if (rc) return rc;
  return fl_launch_spread_tiles(ctx, fl_level_planes(det, g, g.spread_off), det->M, n_frames, g.w, g.h, g.T, tiles, tstride);
}

// ---- single-image stage entry points ----------------------------------------------------------
template <typename F>
static int run_stage(fl_context *ctx, const void *in, size_t in_bytes, void *out, size_t out_bytes, size_t tmp_bytes,
                     int mem, F body)
{
  FL_HIP(ctx, hipSetDevice(ctx->device));
  const uint8_t *din = (const uint8_t *)in;
  uint8_t *dout = (uint8_t *)out, *dtmp = nullptr;
  void *s = nullptr;
  size_t need = fl_align(tmp_bytes, 256) + (mem == FL_MEM_HOST ? fl_align(in_bytes, 256) + fl_align(out_bytes, 256) : 0);
  if (need) {
    int rc = fl_scratch(ctx, need, &s);
    if (rc) return rc;
  }
  dtmp = (uint8_t *)s;
  if (mem == FL_MEM_HOST) {
    uint8_t *b = (uint8_t *)s + fl_align(tmp_bytes, 256);
    FL_HIP(ctx, hipMemcpyAsync(b, in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    din = b;
    dout = b + fl_align(in_bytes, 256);
  }
  int rc = body(din, dout, dtmp);
  if (rc) return rc;
  if (mem == FL_MEM_HOST) {
    FL_HIP(ctx, hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return FL_OK;
}

extern "C" int fl_quantized_orientations(fl_context *ctx, const uint8_t *bgr, int w, int h, float weak_threshold,
                                         uint8_t *dst, int mem)
{
  if (!ctx || !bgr || !dst || w < 3 || h < 3) return FL_ERR_INVALID;
  return run_stage(ctx, bgr, (size_t)w * h * 3, dst, (size_t)w * h, 0, mem,
                   [&](const uint8_t *i, uint8_t *o, uint8_t *) {
                     return fl_launch_quantized_orientations(ctx, i, 0, o, 0, 1, w, h, weak_threshold);
                   });
}

extern "C" int fl_quantized_normals(fl_context *ctx, const uint16_t *depth, int w, int h, int distance_threshold,
                                    int difference_threshold, uint8_t *dst, int mem)
{
  if (!ctx || !depth || !dst || w <= 0 || h <= 0) return FL_ERR_INVALID;
  return run_stage(ctx, depth, (size_t)w * h * 2, dst, (size_t)w * h, (size_t)w * h, mem,
                   [&](const uint8_t *i, uint8_t *o, uint8_t *) {
                     return fl_launch_quantized_normals(ctx, (const uint16_t *)i, 0, o, 0, nullptr, 0, 1, w, h,
                                                        distance_threshold, difference_threshold);
                   });
}

extern "C" int fl_pyrdown_bgr(fl_context *ctx, const uint8_t *src, int w, int h, uint8_t *dst, int mem)
{
  if (!ctx || !src || !dst || w < 2 || h < 2) return FL_ERR_INVALID;
  return run_stage(ctx, src, (size_t)w * h * 3, dst, (size_t)(w / 2) * (h / 2) * 3, 0, mem,
                   [&](const uint8_t *i, uint8_t *o, uint8_t *) { return fl_launch_pyrdown_bgr(ctx, i, 0, o, 0, 1, w, h); });
}

// ------------------------------------------------------------------------------------------
// cv::resize(INTER_LINEAR) as CObjRecoLmICP::PrepareInputData applies it to frames that are not 640
// wide (obj_reco_lmicp.cpp:39-45, 229-249).  OpenCV 3.x semantics restated in oracle/frontend_oracle.c
// (orc_resize_linear_*): exact 2x2 decimation takes the INTER_AREA fast path, everything else two taps
// per axis -- 11-bit fixed point for 8-bit data, float for 16-bit data.  One thread per output pixel;
// this stage runs once per frame ahead of the batch and is HBM-bound (reads 4 source pixels).
struct FlResizeTap { int ofs; float w0, w1; };
__device__ __forceinline__ FlResizeTap fl_resize_tap(int d, int ssize, double scale)
{
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= ssize - 1) { f = 0.f; s = ssize - 1; }
  return {s, 1.f - f, f};
}
__device__ __forceinline__ int fl_sat_short(float v)
{
  const int r = (int)rintf(v);                           // saturate_cast<short>(float): round half even
  return r < -32768 ? -32768 : r > 32767 ? 32767 : r;
}

template <typename T, int CN>
__global__ __launch_bounds__(256) void k_resize_linear(const T *__restrict__ src, int sw, int sh, T *__restrict__ dst, int dw,
                                                       int dh, double scale_x, double scale_y, int area2)
{
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  if (area2) {                                           // (a + b + c + d + 2) >> 2
    const T *s0 = src + ((size_t)(2 * y) * sw + 2 * x) * CN, *s1 = s0 + (size_t)sw * CN;
#pragma unroll
    for (int c = 0; c < CN; ++c) dst[((size_t)y * dw + x) * CN + c] = (T)(((int)s0[c] + s0[CN + c] + s1[c] + s1[CN + c] + 2) >> 2);
    return;
  }
  const FlResizeTap ty = fl_resize_tap(y, sh, scale_y), tx = fl_resize_tap(x, sw, scale_x);
  const int y0 = ty.ofs, y1 = min(ty.ofs + 1, sh - 1), x0 = tx.ofs, x1 = min(tx.ofs + 1, sw - 1);
  const T *r0 = src + (size_t)y0 * sw * CN, *r1 = src + (size_t)y1 * sw * CN;
  if (sizeof(T) == 1) {
    const int a0 = fl_sat_short(tx.w0 * 2048.f), a1 = fl_sat_short(tx.w1 * 2048.f);
    const int b0 = fl_sat_short(ty.w0 * 2048.f), b1 = fl_sat_short(ty.w1 * 2048.f);
#pragma unroll
    for (int c = 0; c < CN; ++c) {
      const int S0 = (int)r0[x0 * CN + c] * a0 + (int)r0[x1 * CN + c] * a1;
      const int S1 = (int)r1[x0 * CN + c] * a0 + (int)r1[x1 * CN + c] * a1;
      dst[((size_t)y * dw + x) * CN + c] = (T)((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2);
    }
  } else {
#pragma unroll
    for (int c = 0; c < CN; ++c) {
      float S0 = (float)r0[x0 * CN + c] * tx.w0;
      S0 = S0 + (float)r0[x1 * CN + c] * tx.w1;
      float S1 = (float)r1[x0 * CN + c] * tx.w0;
      S1 = S1 + (float)r1[x1 * CN + c] * tx.w1;
      float v = S0 * ty.w0;
      v = v + S1 * ty.w1;
      const int r = (int)rintf(v);
      dst[((size_t)y * dw + x) * CN + c] = (T)(r < 0 ? 0 : r > 65535 ? 65535 : r);
    }
  }
}

template <typename T, int CN>
static int fl_resize_linear(fl_context *ctx, const T *src, int sw, int sh, T *dst, int dw, int dh, int mem)
{
  if (!ctx || !src || !dst || sw < 1 || sh < 1 || dw < 1 || dh < 1) return FL_ERR_INVALID;
  const double scale_x = (double)sw / dw, scale_y = (double)sh / dh;
  const int area2 = fabs(scale_x - 2.0) < 2.220446049250313e-16 && fabs(scale_y - 2.0) < 2.220446049250313e-16;
  return run_stage(ctx, src, (size_t)sw * sh * CN * sizeof(T), dst, (size_t)dw * dh * CN * sizeof(T), 0, mem,
                   [&](const uint8_t *i, uint8_t *o, uint8_t *) {
                     hipLaunchKernelGGL((k_resize_linear<T, CN>), dim3((dw + 63) / 64, (dh + 3) / 4), dim3(256), 0, ctx->stream,
                                        (const T *)i, sw, sh, (T *)o, dw, dh, scale_x, scale_y, area2);
                     FL_HIP(ctx, hipGetLastError());
                     return (int)FL_OK;
                   });
}

// device-to-device launchers for the pipeline (fl_recognize_batch_zoom)
int fl_launch_resize_linear_bgr8(fl_context *ctx, const uint8_t *src, int sw, int sh, uint8_t *dst, int dw, int dh)
{
  return fl_resize_linear<uint8_t, 3>(ctx, src, sw, sh, dst, dw, dh, FL_MEM_DEVICE);
}
int fl_launch_resize_linear_u16(fl_context *ctx, const uint16_t *src, int sw, int sh, uint16_t *dst, int dw, int dh)
{
  return fl_resize_linear<uint16_t, 1>(ctx, src, sw, sh, dst, dw, dh, FL_MEM_DEVICE);
}

extern "C" int fl_resize_linear_bgr8(fl_context *ctx, const uint8_t *src, int sw, int sh, uint8_t *dst, int dw, int dh, int mem)
{
  return fl_resize_linear<uint8_t, 3>(ctx, src, sw, sh, dst, dw, dh, mem);
}

extern "C" int fl_resize_linear_u16(fl_context *ctx, const uint16_t *src, int sw, int sh, uint16_t *dst, int dw, int dh, int mem)
{
  return fl_resize_linear<uint16_t, 1>(ctx, src, sw, sh, dst, dw, dh, mem);
}

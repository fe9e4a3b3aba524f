// Training augmentation of the detection crops on the device (include/mmmot_hip.h: mmmot_crop_augment; DESIGN
// section 18): per crop torchvision's ``resized_crop(img, top, left, h, w, (S, S), BILINEAR)`` - for a PIL image
// ``img.crop((left, top, left + w, top + h)).resize((S, S), BILINEAR)`` - then ``hflip`` when the row says so, then
// to_tensor + normalize: the train_transform of the reference (utils/build_util.py:110-144) behind the 8-bit S x S crop
// that csrc/crop_resize.hip makes.  One launch for all L crops, no scratch buffer.
//
// The region lies inside the S x S crop and is never larger than the output, so nothing is padded and the triangle
// filter has support 1: at most 3 taps per output index in either pass (csrc/crop_coeff.h, Pillow's arithmetic).
//
// Workgroup = CA_TR output rows of one crop, all S columns, 256 threads:
//   A  thread x computes the horizontal taps of output column x, 16 threads the vertical taps of the tile's rows, all the
//      3 x 256 table byte -> normalised float (the two fp32 divisions once per byte value, not once per pixel) - into LDS;
//   B  the source rows the tile needs - at most CA_TR + 2, (CA_TR - 1) h / S + 3 - are staged into LDS as aligned dwords;
//   C  horizontal pass over those rows -> the 8-bit intermediate rows in LDS, each computed once per tile;
//   D  vertical pass, flip, table look-up, store.  S % 4 == 0 (and aligned outputs): a thread makes 4 pixels x 3
//      channels and stores one float4 per channel plane and three dwords of bytes, a wave 1 KB lines; else one pixel.
// Bound by the fp32 store (12 S^2 bytes per crop); the source is L * S^2 * 3 bytes read through L2.
#include "crop_coeff.h"

#define CA_TR 16                     // output rows per workgroup
#define CA_ROWS (CA_TR + 4)          // staged source rows (needed: <= CA_TR + 2)
#define CA_SRC_DW 196                // dwords per staged source row: 3 bytes misalignment + 256 * 3, and the 3-dword reads
#define CA_H_DW 192                  // dwords per intermediate row: 256 * 3 bytes
#define CA_ROUND (1 << (CR_PREC - 1))

template <int VEC>
__global__ __launch_bounds__(256) void ca_augment_kernel(const unsigned char* __restrict__ crops,
                                                         const int* __restrict__ params, int S, long total_bytes,
                                                         const float* __restrict__ ms, float* __restrict__ out,
                                                         unsigned char* __restrict__ out_u8) {
  __shared__ int4 hc[256];                       // per output column: first tap, 3 weights
  __shared__ int4 vc[CA_TR];                     // per output row of the tile: first tap, 3 weights
  __shared__ int vcnt[CA_TR];                    // ... and its number of taps
  __shared__ float lut[3 * 256];                 // channel, byte -> normalised float
  __shared__ unsigned src[CA_ROWS * CA_SRC_DW];  // staged source rows, from the aligned address at or below the region
  __shared__ unsigned hbuf[CA_ROWS * CA_H_DW];   // horizontally resampled rows [x][c] bytes
  const int l = blockIdx.x, oy0 = blockIdx.y * CA_TR, tid = threadIdx.x;
  const int trn = S - oy0 < CA_TR ? S - oy0 : CA_TR;
  const int* p = params + (long)l * 5;
  // the table is validated on the host; the clamp keeps a bad one inside the crop all the same
  int top = p[0], left = p[1], h = p[2], w = p[3];
  const bool flip = p[4] != 0;
  top = top < 0 ? 0 : (top > S - 1 ? S - 1 : top);
  left = left < 0 ? 0 : (left > S - 1 ? S - 1 : left);
  h = h < 1 ? 1 : (h > S - top ? S - top : h);
  w = w < 1 ? 1 : (w > S - left ? S - left : w);

  // ---- A: coefficients and the normalisation table ----
  if (tid < S) {
    int b[2];
    int* k = (int*)&hc[tid];
    cr_coeffs(w, S, tid, 3, b, k + 1);
    k[0] = b[0];
  }
  const int vt = 255 - tid;  // the last threads: not the ones of a narrow crop's columns
  if (vt < trn) {
    int b[2];
    int* k = (int*)&vc[vt];
    cr_coeffs(h, S, oy0 + vt, 3, b, k + 1);
    k[0] = b[0];
    vcnt[vt] = b[1];
  }
  if (out)
    for (int i = tid; i < 3 * 256; i += 256) lut[i] = cr_norm(i & 255, ms[i >> 8], ms[3 + (i >> 8)]);
  __syncthreads();

  // ---- B: stage source rows [ymin0, ymin0 + nrows) of the region, columns [left, left + w) ----
  const int ymin0 = vc[0].x;
  int nrows = vc[trn - 1].x + vcnt[trn - 1] - ymin0;
  nrows = nrows > CA_ROWS ? CA_ROWS : nrows;
  const uintptr_t p0 = (uintptr_t)crops, p1 = p0 + total_bytes;
  const long row0 = (long)l * S + top + ymin0;  // image row of staged row 0, counted over all crops
  const int ndw = (w * 3 + 6) >> 2;             // dwords that cover 3 w bytes from any misalignment: <= 193
  for (int idx = tid; idx < nrows * ndw; idx += 256) {
    const int j = idx / ndw, k = idx - j * ndw;
    const uintptr_t a = ((p0 + ((row0 + j) * S + left) * 3) & ~(uintptr_t)3) + 4 * k;
    unsigned d = 0;
    if (a >= p0 && a + 4 <= p1) {
      d = *(const unsigned*)a;
    } else {  // the first or last dword of the whole tensor: only the bytes that belong to it
      for (int b = 0; b < 4; ++b)
        if (a + b >= p0 && a + b < p1) d |= (unsigned)*(const unsigned char*)(a + b) << (8 * b);
    }
    src[j * CA_SRC_DW + k] = d;
  }
  __syncthreads();

  // ---- C: horizontal pass, one (row, column) per thread and step: 9 bytes from 3 dwords ----
  for (int idx = tid; idx < nrows * S; idx += 256) {
    const int j = idx / S, ox = idx - j * S;
    const int4 c = hc[ox];
    const unsigned o = (unsigned)((p0 + ((row0 + j) * S + left) * 3) & 3) + c.x * 3;  // byte offset in the staged row
    const unsigned* r = src + j * CA_SRC_DW + (o >> 2);
    const unsigned d0 = r[0], d1 = r[1], d2 = r[2], sh = (o & 3) * 8;
    const unsigned q0 = (unsigned)((((unsigned long long)d1 << 32) | d0) >> sh);  // bytes 0..3 of the 9
    const unsigned q1 = (unsigned)((((unsigned long long)d2 << 32) | d1) >> sh);  // bytes 4..7
    const unsigned q2 = d2 >> sh;                                                 // byte 8
    // tap i, channel ch = byte 3 i + ch; weights behind the last tap are zero
    const int a0 = CA_ROUND + (int)(q0 & 255) * c.y + (int)(q0 >> 24) * c.z + (int)((q1 >> 16) & 255) * c.w;
    const int a1 = CA_ROUND + (int)((q0 >> 8) & 255) * c.y + (int)(q1 & 255) * c.z + (int)(q1 >> 24) * c.w;
    const int a2 = CA_ROUND + (int)((q0 >> 16) & 255) * c.y + (int)((q1 >> 8) & 255) * c.z + (int)(q2 & 255) * c.w;
    unsigned char* hb = (unsigned char*)hbuf + j * (CA_H_DW * 4) + ox * 3;
    hb[0] = (unsigned char)cr_clip8(a0);  // the 8-bit intermediate image of the two-pass resize
    hb[1] = (unsigned char)cr_clip8(a1);
    hb[2] = (unsigned char)cr_clip8(a2);
  }
  __syncthreads();

  // ---- D: vertical pass, flip, normalise, store ----
  const int G = S / VEC;
  for (int idx = tid; idx < trn * G; idx += 256) {
    const int r = idx / G, g = idx - r * G, oy = oy0 + r;
    const int4 c = vc[r];
    const int kv[3] = {c.y, c.z, c.w};
    const int j0 = c.x - ymin0;
    const int gr = flip ? G - 1 - g : g;  // out[.., x] = res[.., S - 1 - x]
    int v[VEC * 3];
#pragma unroll
    for (int b = 0; b < VEC * 3; ++b) v[b] = CA_ROUND;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int row = j0 + t < CA_ROWS ? j0 + t : CA_ROWS - 1;  // rows behind the last tap carry weight zero
      if (VEC == 4) {
        const unsigned* hp = hbuf + row * CA_H_DW + gr * 3;
        const unsigned d[3] = {hp[0], hp[1], hp[2]};
#pragma unroll
        for (int b = 0; b < 12; ++b) v[b] += (int)((d[b >> 2] >> (8 * (b & 3))) & 255) * kv[t];
      } else {
        const unsigned char* hp = (const unsigned char*)hbuf + row * (CA_H_DW * 4) + gr * 3;
#pragma unroll
        for (int b = 0; b < 3; ++b) v[b] += (int)hp[b] * kv[t];
      }
    }
#pragma unroll
    for (int b = 0; b < VEC * 3; ++b) v[b] = cr_clip8(v[b]);
    if (VEC == 4 && flip) {  // the four pixels of the group change places as well
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        int t = v[ch]; v[ch] = v[9 + ch]; v[9 + ch] = t;
        t = v[3 + ch]; v[3 + ch] = v[6 + ch]; v[6 + ch] = t;
      }
    }
    const long pix = ((long)l * S + oy) * S + (long)g * VEC;  // first output pixel of the group, [l][oy][x]
    if (out_u8) {
      if (VEC == 4) {
        unsigned* o8 = (unsigned*)(out_u8 + pix * 3);
#pragma unroll
        for (int m = 0; m < 3; ++m)
          o8[m] = (unsigned)v[4 * m] | ((unsigned)v[4 * m + 1] << 8) | ((unsigned)v[4 * m + 2] << 16) |
                  ((unsigned)v[4 * m + 3] << 24);
      } else {
#pragma unroll
        for (int b = 0; b < 3; ++b) out_u8[pix * 3 + b] = (unsigned char)v[b];
      }
    }
    if (out) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        float* o = out + (((long)l * 3 + ch) * S + oy) * S + (long)g * VEC;
        if (VEC == 4)
          *(float4*)o = make_float4(lut[ch * 256 + v[ch]], lut[ch * 256 + v[3 + ch]], lut[ch * 256 + v[6 + ch]],
                                    lut[ch * 256 + v[9 + ch]]);
        else
          *o = lut[ch * 256 + v[ch]];
      }
    }
  }
}

extern "C" int mmmot_crop_augment(const unsigned char* crops_u8, const int* params, int L, int S, const float* mean_std,
                                  float* out, unsigned char* out_u8, void* stream) {
  if (!crops_u8 || !params || (!out && !out_u8) || (out && !mean_std) || L < 1 || S < 1 || S > 256) return MMMOT_EINVAL;
  const long total = (long)L * S * S * 3;
  const dim3 grid(L, (S + CA_TR - 1) / CA_TR);
  const bool vec = S % 4 == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)out_u8 & 3) == 0;
  if (vec)
    hipLaunchKernelGGL(ca_augment_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, crops_u8, params, S, total,
                       mean_std, out, out_u8);
  else
    hipLaunchKernelGGL(ca_augment_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, crops_u8, params, S, total,
                       mean_std, out, out_u8);
  return mm_check(hipGetLastError());
}

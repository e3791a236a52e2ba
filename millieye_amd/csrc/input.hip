// Input producer on the GPU: what module3_our_dataset/utils/datasets.py does per frame on
// the CPU between the decoded jpg / radar pickle and the batch tensors Network.forward takes.
//   me_image_pad_resize_u8_f32  ToTensor (u8 HWC -> f32 CHW / 255, datasets.py:203) + pad_to_square (:16-27, :211) +
//                               resize(img, S) = F.interpolate(nearest) (:30-32, :317), one pass, one write.
//   me_image_batch_pad_resize_flip_u8_f32
//                               the same for a ragged batch (frames of different sizes packed in one uint8 buffer, one
//                               descriptor per frame), one launch; with the stage-2 flip (module2_mixed/utils/datasets.py:275-304).
//   me_image_batch_formats_u8_f32
//                               the ragged batch with a pixel format per frame (RGB, BGR, NV12, YUYV): the frames a camera
//                               or a decoder hands over, without the host's conversion to RGB (run_mp.py:50,114).
//   me_image_batch_area_u8_f32  the same ragged batch with F.interpolate(mode="area") for the resize: an option the reference's
//                               scripts do not have, pinned to torch's float64 area interpolation (exact integer sums).
//   me_image_batch_letterbox_u8_f32
//                               the same ragged batch letterboxed to a rectangular H x W canvas (letterbox.h), for the
//                               rectangular network input; torch's F.pad + F.interpolate(nearest) bit for bit.
//   me_image_batch_surfaces_u8_f32
//                               the letterbox and the area kernel reading every frame through a descriptor of its own
//                               (buffer, offset, row pitch, NV12 chroma plane): pitched, cropped and device-resident frames.
//   me_radar_heatmap_rect_f32   me_radar_heatmap_f32 with a rectangular mh x mw output (the bins letterboxed the same way).
//   me_radar_heatmap_f32        plot_radar_heatmap (:59-106: three np.histogram2d in float64, per-bin means, range
//                               normalisation) + ToTensor().float() (:267) + pad_to_square (:270) +
//                               F.interpolate(bilinear, align_corners=True) to the map size (:318-321).
// Both are HBM/latency-trivial (a 1600x900 frame is 4.3 MB in, 2 MB out); the point is that the batch never
// exists on the host and the 3 histograms + resize per frame leave the DataLoader's critical path.
#include <type_traits>

#include "common.h"
#include "letterbox.h"

// every product / sum below is a separately rounded IEEE operation in the reference (numpy float64, aten float32
// scalar kernels): no fused multiply-add contraction
#pragma clang fp contract(off)

namespace {

// ---- image: u8 HWC -> padded square -> nearest resize -> f32 CHW -------------------------------------------
// flip: the padded square is mirrored left-right before the resize (module2_mixed/utils/datasets.py:143-146,
// utils/augmentations.py: horisontal_flip runs on the padded tensor, the resize in collate_fn afterwards)
__global__ __launch_bounds__(256) void image_pad_resize_kernel(const unsigned char* __restrict__ src, int h, int w,
                                                               float* __restrict__ dst, int S, int flip) {
  const int P = h > w ? h : w;                 // padded side
  const int diff = h > w ? h - w : w - h;
  const int pad1 = diff / 2;                   // upper / left padding (datasets.py:20)
  const int pad_top = h <= w ? pad1 : 0, pad_left = h <= w ? 0 : pad1;
  // torch nearest (aten UpSampleKernel nearest_idx): src = min(int(floorf(dst * scale)), in - 1),
  // scale = float(in) / out; identity when in == out
  const float scale = (float)P / (float)S;
  const int total = S * S;
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const int y = idx / S, x = idx - y * S;
    int py = P == S ? y : (int)floorf((float)y * scale);
    int px = P == S ? x : (int)floorf((float)x * scale);
    py = py < P - 1 ? py : P - 1;
    px = px < P - 1 ? px : P - 1;
    if (flip) px = P - 1 - px;
    const int sy = py - pad_top, sx = px - pad_left;
    float r = 0.f, g = 0.f, b = 0.f;  // pad_value 0 (datasets.py:211)
    if ((unsigned)sy < (unsigned)h && (unsigned)sx < (unsigned)w) {
      const unsigned char* p = src + ((size_t)sy * w + sx) * 3;
      r = (float)p[0] / 255.f;  // ToTensor: .float().div(255) - IEEE division
      g = (float)p[1] / 255.f;
      b = (float)p[2] / 255.f;
    }
    dst[idx] = r;
    dst[total + idx] = g;
    dst[2 * total + idx] = b;
  }
}

// ---- ragged batch: every frame of a batch in one launch ------------------------------------------------------
// grid (tiles, n): blockIdx.y = frame, each thread writes 4 consecutive output pixels of one row as float4 per channel
// (S % 4 == 0; otherwise one pixel per thread).  Per pixel the index arithmetic, the division and the pad / flip rules are
// those of image_pad_resize_kernel above, operation for operation: the two produce the same bits.
constexpr int kBatchPix = 4 * 256;  // output pixels per workgroup and tile

__global__ __launch_bounds__(256) void image_batch_pad_resize_kernel(const unsigned char* __restrict__ src,
                                                                     long long src_bytes,
                                                                     const long long* __restrict__ desc,
                                                                     float* __restrict__ dst, int S) {
  const int f = blockIdx.y;
  const long long off = desc[4 * f];
  const int h = (int)desc[4 * f + 1], w = (int)desc[4 * f + 2], flip = desc[4 * f + 3] != 0;
  // a descriptor that does not lie inside the packed buffer reads nothing: the frame comes out as padding
  const bool valid = h > 0 && w > 0 && off >= 0 && off + (long long)h * w * 3 <= src_bytes;
  const int P = h > w ? h : w;
  const int diff = h > w ? h - w : w - h;
  const int pad1 = diff / 2;
  const int pad_top = h <= w ? pad1 : 0, pad_left = h <= w ? 0 : pad1;
  const float scale = (float)P / (float)S;
  const int total = S * S;
  const unsigned char* frame = src + (valid ? off : 0);
  float* out = dst + (size_t)f * 3 * total;
  auto pixel = [&](int y, int x, float& r, float& g, float& b) {
    int py = P == S ? y : (int)floorf((float)y * scale);
    int px = P == S ? x : (int)floorf((float)x * scale);
    py = py < P - 1 ? py : P - 1;
    px = px < P - 1 ? px : P - 1;
    if (flip) px = P - 1 - px;
    const int sy = py - pad_top, sx = px - pad_left;
    r = 0.f, g = 0.f, b = 0.f;
    if (valid && (unsigned)sy < (unsigned)h && (unsigned)sx < (unsigned)w) {
      const unsigned char* p = frame + ((size_t)sy * w + sx) * 3;
      r = (float)p[0] / 255.f;
      g = (float)p[1] / 255.f;
      b = (float)p[2] / 255.f;
    }
  };
  if ((S & 3) == 0) {
    for (int base = blockIdx.x * kBatchPix + threadIdx.x * 4; base < total; base += gridDim.x * kBatchPix) {
      const int y = base / S, x0 = base - y * S;  // the 4 pixels share row y (S % 4 == 0, base % 4 == 0)
      float4 r4, g4, b4;
      pixel(y, x0, r4.x, g4.x, b4.x);
      pixel(y, x0 + 1, r4.y, g4.y, b4.y);
      pixel(y, x0 + 2, r4.z, g4.z, b4.z);
      pixel(y, x0 + 3, r4.w, g4.w, b4.w);
      *reinterpret_cast<float4*>(out + base) = r4;
      *reinterpret_cast<float4*>(out + total + base) = g4;
      *reinterpret_cast<float4*>(out + 2 * total + base) = b4;
    }
  } else {
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
      const int y = idx / S, x = idx - y * S;
      float r, g, b;
      pixel(y, x, r, g, b);
      out[idx] = r;
      out[total + idx] = g;
      out[2 * total + idx] = b;
    }
  }
}

// ---- ragged batch with a pixel format per frame --------------------------------------------------------------
// image_batch_pad_resize_kernel with desc [n,5] = (byte offset, h, w, flip, ME_PIXFMT_*): what a camera or a decoder hands
// over (run_mp.py:50 reads BGR from cv2.VideoCapture, USB cameras give YUYV, video decoders NV12) goes to the RGB planes
// without a host conversion pass.  h, w are the picture's size in pixels.  The format is uniform per blockIdx.y, so the
// switch below is a scalar branch; everything around the fetch is the kernel above, operation for operation.
// YUV -> RGB: the integer limited-range BT.601 conversion of cv2.cvtColor(COLOR_YUV2RGB_NV12 / _YUY2), 20 fractional bits;
// int32 holds every intermediate (about -161 M .. +560 M); >> is arithmetic.  Chroma is not interpolated.
__device__ inline int clamp_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ inline void yuv_to_rgb(int Y, int U, int V, int& r, int& g, int& b) {
  const int y = (Y > 16 ? Y - 16 : 0) * 1220542, u = U - 128, v = V - 128;
  r = clamp_u8((y + (1 << 19) + 1673527 * v) >> 20);
  g = clamp_u8((y + (1 << 19) - 852492 * v - 409993 * u) >> 20);
  b = clamp_u8((y + (1 << 19) + 2116026 * u) >> 20);
}

// The validity rule of a [n,5] descriptor row: a frame that does not lie inside the packed buffer, names no format or breaks
// its format's parity rule.  The size test divides, so that no product of descriptor values can overflow.
__device__ inline bool format_frame_valid(long long off, long long h64, long long w64, long long fmt64, long long src_bytes) {
  bool valid = h64 > 0 && w64 > 0 && h64 <= (1ll << 30) && w64 <= (1ll << 30) && off >= 0 && off <= src_bytes;
  const long long avail = src_bytes - off;
  if (fmt64 == ME_PIXFMT_RGB || fmt64 == ME_PIXFMT_BGR)
    valid = valid && h64 <= avail / (3 * w64);
  else if (fmt64 == ME_PIXFMT_NV12)   // hw + hw/2 = (h/2) rows pairs of 3w bytes
    valid = valid && (h64 & 1) == 0 && (w64 & 1) == 0 && h64 / 2 <= avail / (3 * w64);
  else if (fmt64 == ME_PIXFMT_YUYV)
    valid = valid && (w64 & 1) == 0 && h64 <= avail / (2 * w64);
  else
    valid = false;
  return valid;
}

// 8-bit R, G, B of picture pixel (sy, sx) of a valid frame in format fmt
__device__ inline void fetch_rgb_u8(const unsigned char* __restrict__ frame, int h, int w, int fmt, int sy, int sx, int& ri,
                                    int& gi, int& bi) {
  if (fmt == ME_PIXFMT_RGB || fmt == ME_PIXFMT_BGR) {
    const unsigned char* p = frame + ((size_t)sy * w + sx) * 3;
    ri = fmt == ME_PIXFMT_RGB ? p[0] : p[2];
    gi = p[1];
    bi = fmt == ME_PIXFMT_RGB ? p[2] : p[0];
  } else if (fmt == ME_PIXFMT_NV12) {   // Y plane [h,w], then the interleaved UV plane [h/2,w]
    const unsigned char* uv = frame + (size_t)h * w + (size_t)(sy >> 1) * w + (sx & ~1);
    yuv_to_rgb(frame[(size_t)sy * w + sx], uv[0], uv[1], ri, gi, bi);
  } else {                              // YUYV: rows of Y0 U Y1 V
    const unsigned char* row = frame + (size_t)sy * w * 2;
    const int c = 4 * (sx >> 1);
    yuv_to_rgb(row[2 * sx], row[c + 1], row[c + 3], ri, gi, bi);
  }
}

// ---- surfaces: frames read where they lie ------------------------------------------------------------------------------
// One row of the [n,10] descriptor of me_image_batch_surfaces_u8_f32 = (base, bytes, off, h, w, flip, fmt, pitch, uv_off,
// uv_pitch): a picture inside a buffer [base, base + bytes) of its own, rows `pitch` bytes apart, the NV12 chroma plane at an
// offset and with a pitch of its own.  The letterbox and the area kernel below are instantiated for it (kSurf); only the
// addresses differ from the dense frames, so a surface gives the bits of its pixels copied into a dense frame.
struct Surface {
  const unsigned char* base;
  long long bytes, off, h, w, fmt, pitch, uv_off, uv_pitch;
  int flip;
  bool valid;
};

// The validity rule of a [n,10] row, in 64 bits and with divisions like format_frame_valid: the rows of plane 0 (and of the
// NV12 chroma plane) lie inside [0, bytes).  An invalid surface is never read.
__device__ inline Surface load_surface(const long long* __restrict__ d) {
  Surface s;
  s.base = reinterpret_cast<const unsigned char*>(d[0]);
  s.bytes = d[1], s.off = d[2], s.h = d[3], s.w = d[4], s.flip = d[5] != 0, s.fmt = d[6];
  s.pitch = d[7], s.uv_off = d[8], s.uv_pitch = d[9];
  bool valid = d[0] != 0 && s.bytes > 0 && s.h >= 1 && s.w >= 1 && s.h <= (1ll << 30) && s.w <= (1ll << 30);
  long long row = 1;   // bytes of one row of plane 0
  if (s.fmt == ME_PIXFMT_RGB || s.fmt == ME_PIXFMT_BGR)
    row = 3 * s.w;
  else if (s.fmt == ME_PIXFMT_NV12)
    row = s.w, valid = valid && (s.h & 1) == 0 && (s.w & 1) == 0;
  else if (s.fmt == ME_PIXFMT_YUYV)
    row = 2 * s.w, valid = valid && (s.w & 1) == 0;
  else
    valid = false;
  valid = valid && s.pitch >= row && row <= s.bytes && s.off >= 0 && s.off <= s.bytes - row;
  valid = valid && s.h - 1 <= (s.bytes - row - s.off) / s.pitch;
  if (valid && s.fmt == ME_PIXFMT_NV12) {
    valid = s.uv_pitch >= s.w && s.uv_off >= 0 && s.uv_off <= s.bytes - s.w;
    valid = valid && s.h / 2 - 1 <= (s.bytes - s.w - s.uv_off) / s.uv_pitch;
  }
  // a pitch nobody steps by (a single row) may be any number: keep the address arithmetic small
  if (s.h == 1) s.pitch = row;
  if (s.h == 2) s.uv_pitch = s.w;
  s.valid = valid;
  return s;
}

// fetch_rgb_u8 for a valid surface: 64-bit byte addresses from base
__device__ inline void fetch_rgb_u8(const Surface& s, int fmt, int sy, int sx, int& ri, int& gi, int& bi) {
  const unsigned char* row = s.base + s.off + sy * s.pitch;
  if (fmt == ME_PIXFMT_RGB || fmt == ME_PIXFMT_BGR) {
    const unsigned char* p = row + 3 * sx;
    ri = fmt == ME_PIXFMT_RGB ? p[0] : p[2];
    gi = p[1];
    bi = fmt == ME_PIXFMT_RGB ? p[2] : p[0];
  } else if (fmt == ME_PIXFMT_NV12) {
    const unsigned char* uv = s.base + s.uv_off + (sy >> 1) * s.uv_pitch + (sx & ~1);
    yuv_to_rgb(row[sx], uv[0], uv[1], ri, gi, bi);
  } else {
    const int c = 4 * (sx >> 1);
    yuv_to_rgb(row[2 * sx], row[c + 1], row[c + 3], ri, gi, bi);
  }
}

__global__ __launch_bounds__(256) void image_batch_formats_kernel(const unsigned char* __restrict__ src,
                                                                  long long src_bytes,
                                                                  const long long* __restrict__ desc,
                                                                  float* __restrict__ dst, int S) {
  const int f = blockIdx.y;
  const long long off = desc[5 * f], h64 = desc[5 * f + 1], w64 = desc[5 * f + 2], fmt64 = desc[5 * f + 4];
  const int flip = desc[5 * f + 3] != 0;
  // an invalid descriptor reads nothing: the frame comes out as padding
  const bool valid = format_frame_valid(off, h64, w64, fmt64, src_bytes);
  const int h = valid ? (int)h64 : 1, w = valid ? (int)w64 : 1, fmt = (int)fmt64;
  const int P = h > w ? h : w;
  const int diff = h > w ? h - w : w - h;
  const int pad1 = diff / 2;
  const int pad_top = h <= w ? pad1 : 0, pad_left = h <= w ? 0 : pad1;
  const float scale = (float)P / (float)S;
  const int total = S * S;
  const unsigned char* frame = src + (valid ? off : 0);
  float* out = dst + (size_t)f * 3 * total;
  auto pixel = [&](int y, int x, float& r, float& g, float& b) {
    int py = P == S ? y : (int)floorf((float)y * scale);
    int px = P == S ? x : (int)floorf((float)x * scale);
    py = py < P - 1 ? py : P - 1;
    px = px < P - 1 ? px : P - 1;
    if (flip) px = P - 1 - px;
    const int sy = py - pad_top, sx = px - pad_left;
    r = 0.f, g = 0.f, b = 0.f;
    if (valid && (unsigned)sy < (unsigned)h && (unsigned)sx < (unsigned)w) {
      int ri, gi, bi;
      fetch_rgb_u8(frame, h, w, fmt, sy, sx, ri, gi, bi);
      r = (float)ri / 255.f;
      g = (float)gi / 255.f;
      b = (float)bi / 255.f;
    }
  };
  if ((S & 3) == 0) {
    for (int base = blockIdx.x * kBatchPix + threadIdx.x * 4; base < total; base += gridDim.x * kBatchPix) {
      const int y = base / S, x0 = base - y * S;
      float4 r4, g4, b4;
      pixel(y, x0, r4.x, g4.x, b4.x);
      pixel(y, x0 + 1, r4.y, g4.y, b4.y);
      pixel(y, x0 + 2, r4.z, g4.z, b4.z);
      pixel(y, x0 + 3, r4.w, g4.w, b4.w);
      *reinterpret_cast<float4*>(out + base) = r4;
      *reinterpret_cast<float4*>(out + total + base) = g4;
      *reinterpret_cast<float4*>(out + 2 * total + base) = b4;
    }
  } else {
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
      const int y = idx / S, x = idx - y * S;
      float r, g, b;
      pixel(y, x, r, g, b);
      out[idx] = r;
      out[total + idx] = g;
      out[2 * total + idx] = b;
    }
  }
}

// ---- ragged batch, letterbox to a rectangular canvas ---------------------------------------------------------------
// image_batch_formats_kernel for an output of H x W.  With a = H / gcd(H, W), b = W / gcd(H, W) the padded rectangle is the
// smallest (a k) x (b k) that holds the picture: k = max(ceil(h / a), ceil(w / b)) in 64 bits, Ph = a k, Pw = b k, so that
// Ph / H == Pw / W exactly; floor(diff / 2) of the padding goes in front on each axis, the rest behind (letterbox.h).  Then
// the nearest rule per axis.  H == W gives a = b = 1, Ph = Pw = max(h, w): the operations, and the bits, of image_batch_formats_kernel.
// kSurf: desc is [n,10], one Surface per frame, and src / src_bytes are not used (me_image_batch_surfaces_u8_f32).
template <bool kSurf>
__global__ __launch_bounds__(256) void image_batch_letterbox_kernel(const unsigned char* __restrict__ src,
                                                                    long long src_bytes,
                                                                    const long long* __restrict__ desc,
                                                                    float* __restrict__ dst, int H, int W, int a, int b) {
  const int f = blockIdx.y;
  Surface sf{};
  if constexpr (kSurf) sf = load_surface(desc + 10 * f);
  const long long off = kSurf ? sf.off : desc[5 * f], h64 = kSurf ? sf.h : desc[5 * f + 1];
  const long long w64 = kSurf ? sf.w : desc[5 * f + 2], fmt64 = kSurf ? sf.fmt : desc[5 * f + 4];
  const int flip = kSurf ? sf.flip : desc[5 * f + 3] != 0;
  bool valid = kSurf ? sf.valid : format_frame_valid(off, h64, w64, fmt64, src_bytes);
  const LetterboxGeom geo = letterbox_geom(valid ? (int)h64 : 1, valid ? (int)w64 : 1, a, b);
  valid = valid && geo.ok;
  const int h = valid ? (int)h64 : 1, w = valid ? (int)w64 : 1, fmt = (int)fmt64;
  const int Ph = geo.Ph, Pw = geo.Pw, pad_top = geo.top, pad_left = geo.left;
  const float scale_y = (float)Ph / (float)H, scale_x = (float)Pw / (float)W;
  const int total = H * W;
  const unsigned char* frame = src + (valid ? off : 0);
  float* out = dst + (size_t)f * 3 * total;
  auto pixel = [&](int y, int x, float& r, float& g, float& b) {
    int py = Ph == H ? y : (int)floorf((float)y * scale_y);
    int px = Pw == W ? x : (int)floorf((float)x * scale_x);
    py = py < Ph - 1 ? py : Ph - 1;
    px = px < Pw - 1 ? px : Pw - 1;
    if (flip) px = Pw - 1 - px;
    const int sy = py - pad_top, sx = px - pad_left;
    r = 0.f, g = 0.f, b = 0.f;
    if (valid && (unsigned)sy < (unsigned)h && (unsigned)sx < (unsigned)w) {
      int ri, gi, bi;
      if constexpr (kSurf)
        fetch_rgb_u8(sf, fmt, sy, sx, ri, gi, bi);
      else
        fetch_rgb_u8(frame, h, w, fmt, sy, sx, ri, gi, bi);
      r = (float)ri / 255.f;
      g = (float)gi / 255.f;
      b = (float)bi / 255.f;
    }
  };
  if ((W & 3) == 0) {
    for (int base = blockIdx.x * kBatchPix + threadIdx.x * 4; base < total; base += gridDim.x * kBatchPix) {
      const int y = base / W, x0 = base - y * W;  // the 4 pixels share row y (W % 4 == 0, base % 4 == 0)
      float4 r4, g4, b4;
      pixel(y, x0, r4.x, g4.x, b4.x);
      pixel(y, x0 + 1, r4.y, g4.y, b4.y);
      pixel(y, x0 + 2, r4.z, g4.z, b4.z);
      pixel(y, x0 + 3, r4.w, g4.w, b4.w);
      *reinterpret_cast<float4*>(out + base) = r4;
      *reinterpret_cast<float4*>(out + total + base) = g4;
      *reinterpret_cast<float4*>(out + 2 * total + base) = b4;
    }
  } else {
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
      const int y = idx / W, x = idx - y * W;
      float r, g, b;
      pixel(y, x, r, g, b);
      out[idx] = r;
      out[total + idx] = g;
      out[2 * total + idx] = b;
    }
  }
}

// ---- ragged batch, area-averaging resize -----------------------------------------------------------------------
// image_batch_formats_kernel with resize(img, S) = F.interpolate(mode="area") in place of the reference's nearest resize
// (utils/datasets.py:30-32, :317): adaptive average pooling of the padded, optionally mirrored square, in exact integers.
// Output index i covers the padded indices [floor(i P / S), ceil((i + 1) P / S)) on each axis (64-bit products); per channel
// sum = the int32 sum of the window's uint8 values (padding adds 0 and counts), cnt = the window's area and the output is
// (float)sum / (float)(255 * cnt), one IEEE division.  P <= 255 S keeps 255 cnt < 2^24, so both operands are exact and the
// quotient is the correctly rounded one; a frame beyond that is invalid and comes out all zero.  Formats go through
// yuv_to_rgb pixel by pixel BEFORE the sum (the clamps do not commute with it).
// Unlike the nearest kernels this one reads every source byte.  grid (S, n): a workgroup owns one output row of one frame.
// Its source rows are read 16 (NV12: 8 + 8) bytes per lane, coalesced along the row, each lane keeping the column sums of
// its bytes over the window's rows in registers (the vertical half, no cross-lane traffic); the column sums go to LDS once
// and the horizontal half adds each output's window from there.  Row starts are arbitrary byte addresses (3w-, 2w- and
// w-byte rows, frames back to back): the loads are unaligned 16-byte loads, which global memory serves on gfx9 and later;
// only a load that would end behind src_bytes falls back to guarded byte loads.  A row wider than the LDS holds is walked in
// segments of whole output windows (neighbouring windows may share a column, which is then read twice).
constexpr int kAreaRgbBytes = 4096;   // RGB / BGR: 256 lanes x 16 bytes of one row per segment
constexpr int kAreaYuvPix = 2048;     // YUV: 256 lanes x 8 pixels per segment, one LDS plane per channel
constexpr int kAreaLds = 3 * kAreaYuvPix;

// N bytes at src + at as little-endian dwords.  kWide: one unaligned N-byte load, for a caller that knows at + N <= src_bytes;
// otherwise byte loads, and a byte at or behind src_bytes reads as 0.
template <int N, bool kWide>
__device__ inline void load_bytes(const unsigned char* __restrict__ src, long long at, long long src_bytes,
                                  unsigned (&v)[N / 4]) {
  if (kWide) {
    __builtin_memcpy(v, src + at, N);
  } else {
#pragma unroll
    for (int d = 0; d < N / 4; ++d) {
      unsigned x = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (at + 4 * d + j < src_bytes) x |= (unsigned)src[at + 4 * d + j] << (8 * j);
      v[d] = x;
    }
  }
}

// kSurf (me_image_batch_surfaces_u8_f32): desc is [n,10], one Surface per frame.  The rows of a frame are then `pitch` bytes
// apart (the NV12 chroma rows `uv_pitch`, from `uv_off`), and the bound of the wide loads is the frame's own buffer.  A lane's
// 16 bytes may run over the picture's last column into pitch padding or a neighbouring picture, as they run into the next row
// of a dense frame: those column sums lie behind sx1 - sx0 in cs and the horizontal half never adds them.
template <bool kSurf>
__global__ __launch_bounds__(256) void image_batch_area_kernel(const unsigned char* __restrict__ src_, long long src_bytes_,
                                                               const long long* __restrict__ desc,
                                                               float* __restrict__ dst, int S) {
  __shared__ int cs[kAreaLds];   // column sums of the segment: RGB / BGR by byte of the row, YUV [channel][pixel]
  const int f = blockIdx.y, oy = blockIdx.x, t = threadIdx.x;
  Surface sf{};
  if constexpr (kSurf) sf = load_surface(desc + 10 * f);
  const unsigned char* __restrict__ src = kSurf ? sf.base : src_;   // the loads stay inside [src, src + src_bytes)
  const long long src_bytes = kSurf ? sf.bytes : src_bytes_;
  const long long off = kSurf ? sf.off : desc[5 * f], h64 = kSurf ? sf.h : desc[5 * f + 1];
  const long long w64 = kSurf ? sf.w : desc[5 * f + 2], fmt64 = kSurf ? sf.fmt : desc[5 * f + 4];
  const int flip = kSurf ? sf.flip : desc[5 * f + 3] != 0;
  // the validity rules of image_batch_formats_kernel, and the range rule P <= 255 S.  S < 2^15 bounds h and w by 2^23
  // first, so the byte counts below are products that cannot overflow (that kernel divides instead).
  bool valid = h64 > 0 && w64 > 0 && h64 <= 255ll * S && w64 <= 255ll * S && off >= 0 && off <= src_bytes;
  const long long avail = src_bytes - off, hw = valid ? h64 * w64 : 0;
  if (kSurf)
    valid = valid && sf.valid;
  else if (fmt64 == ME_PIXFMT_RGB || fmt64 == ME_PIXFMT_BGR)
    valid = valid && 3 * hw <= avail;
  else if (fmt64 == ME_PIXFMT_NV12)
    valid = valid && (h64 & 1) == 0 && (w64 & 1) == 0 && hw + hw / 2 <= avail;
  else if (fmt64 == ME_PIXFMT_YUYV)
    valid = valid && (w64 & 1) == 0 && 2 * hw <= avail;
  else
    valid = false;
  const int h = valid ? (int)h64 : 1, w = valid ? (int)w64 : 1, fmt = (int)fmt64;
  const bool yuv = fmt == ME_PIXFMT_NV12 || fmt == ME_PIXFMT_YUYV;
  const int P = h > w ? h : w;
  const int diff = h > w ? h - w : w - h;
  const int pad1 = diff / 2;
  const int pad_top = h <= w ? pad1 : 0, pad_left = h <= w ? 0 : pad1;
  const int total = S * S;
  float* out = dst + (size_t)f * 3 * total + (size_t)oy * S;
  // i P = q S + r.  Every product fits 32 bits for the frames of practice ((S + 1) P < 2^31), where the quotient costs a
  // fraction of the 64-bit one; a run of outputs divides once and steps (q, r) by (P / S, P % S).
  const bool small = (long long)(S + 1) * P < (1ll << 31);
  auto divmod = [&](int i, int& q, int& r) {
    if (small) {
      const unsigned n = (unsigned)i * (unsigned)P;
      q = (int)(n / (unsigned)S), r = (int)(n - (unsigned)q * (unsigned)S);
    } else {
      const long long n = (long long)i * P, qq = n / S;
      q = (int)qq, r = (int)(n - qq * S);
    }
  };
  int qs, rs;
  divmod(1, qs, rs);
  auto win_lo = [&](int i) {
    int q, r;
    divmod(i, q, r);
    return q;
  };
  auto win_hi = [&](int i) {
    int q, r;
    divmod(i + 1, q, r);
    return q + (r > 0);
  };
  const int ay = win_lo(oy), by = win_hi(oy);
  const int sy0 = ay - pad_top > 0 ? ay - pad_top : 0, sy1 = by - pad_top < h ? by - pad_top : h;   // picture rows
  // outputs per segment: a multiple of 4 whose windows span at most TX P / S + 2 <= capacity - 1 pixels (one more when
  // the span is moved to an even start); P <= 255 S leaves room for at least 5
  const int cap = yuv ? kAreaYuvPix : kAreaRgbBytes / 3;
  const int tx = (int)((unsigned)((cap - 3) * S) / (unsigned)P) & ~3;   // (S < 2^15: the product stays under 2^26)
  const int TX = tx < 4 ? 4 : (tx > S ? S : tx);
  const int cfirst = fmt == ME_PIXFMT_BGR ? 2 : 0, cstep = fmt == ME_PIXFMT_BGR ? -1 : 1;
  for (int ox0 = 0; ox0 < S; ox0 += TX) {
    const int ox1 = ox0 + TX < S ? ox0 + TX : S;
    // the segment's padded columns, before the mirror, and the picture columns among them
    const int pa = win_lo(ox0), pb = win_hi(ox1 - 1);
    const int lo = flip ? P - pb : pa, hi = flip ? P - pa : pb;
    int sx0 = lo - pad_left > 0 ? lo - pad_left : 0;
    const int sx1 = hi - pad_left < w ? hi - pad_left : w;
    if (yuv) sx0 &= ~1;   // whole chroma pairs
    const bool any = valid && sy1 > sy0 && sx1 > sx0;
    if (any && !yuv) {
      const int k = 16 * t;
      if (k < 3 * (sx1 - sx0)) {
        // two column sums per register, 16 bits each: a window has at most 256 rows (P <= 255 S), 256 * 255 < 2^16
        unsigned acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0;
        const long long pitch = kSurf ? sf.pitch : 3ll * w;
        long long at = off + sy0 * pitch + 3ll * sx0 + k;
        auto add = [&](const unsigned (&v)[4]) {
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            acc[2 * d] += v[d] & 0x00ff00ffu;              // bytes 0 and 2
            acc[2 * d + 1] += (v[d] >> 8) & 0x00ff00ffu;   // bytes 1 and 3
          }
        };
        // the lane's highest address decides once between wide loads and the guarded byte loads (the buffer's last bytes)
        auto rows = [&](auto wide) {
          constexpr bool kWide = decltype(wide)::value;
          int sy = sy0;
#pragma unroll 1
          for (; kWide && sy + 4 <= sy1; sy += 4, at += 4 * pitch) {   // four rows in flight
            unsigned v0[4], v1[4], v2[4], v3[4];
            load_bytes<16, kWide>(src, at, src_bytes, v0);
            load_bytes<16, kWide>(src, at + pitch, src_bytes, v1);
            load_bytes<16, kWide>(src, at + 2 * pitch, src_bytes, v2);
            load_bytes<16, kWide>(src, at + 3 * pitch, src_bytes, v3);
            add(v0), add(v1), add(v2), add(v3);
          }
          for (; sy < sy1; ++sy, at += pitch) {
            unsigned v0[4];
            load_bytes<16, kWide>(src, at, src_bytes, v0);
            add(v0);
          }
        };
        if (at + (sy1 - 1 - sy0) * pitch + 16 <= src_bytes)
          rows(std::true_type{});
        else
          rows(std::false_type{});
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          cs[k + 4 * d] = (int)(acc[2 * d] & 0xffffu);
          cs[k + 4 * d + 1] = (int)(acc[2 * d + 1] & 0xffffu);
          cs[k + 4 * d + 2] = (int)(acc[2 * d] >> 16);
          cs[k + 4 * d + 3] = (int)(acc[2 * d + 1] >> 16);
        }
      }
    } else if (any) {
      const int k = 8 * t;
      if (k < sx1 - sx0) {
        int acc[24];
#pragma unroll
        for (int j = 0; j < 24; ++j) acc[j] = 0;
        auto add = [&](int j, int Y, int U, int V) {
          int r, g, b;
          yuv_to_rgb(Y, U, V, r, g, b);
          acc[j] += r, acc[8 + j] += g, acc[16 + j] += b;
        };
        if (fmt == ME_PIXFMT_YUYV) {   // rows of Y0 U Y1 V
          const long long pitch = kSurf ? sf.pitch : 2ll * w;
          long long at = off + sy0 * pitch + 2ll * (sx0 + k);
          auto rows = [&](auto wide) {
            for (int sy = sy0; sy < sy1; ++sy, at += pitch) {
              unsigned v[4];
              load_bytes<16, decltype(wide)::value>(src, at, src_bytes, v);
#pragma unroll
              for (int p = 0; p < 4; ++p) {
                const int U = (v[p] >> 8) & 255u, V = v[p] >> 24;
                add(2 * p, v[p] & 255u, U, V);
                add(2 * p + 1, (v[p] >> 16) & 255u, U, V);
              }
            }
          };
          if (at + (sy1 - 1 - sy0) * pitch + 16 <= src_bytes)
            rows(std::true_type{});
          else
            rows(std::false_type{});
        } else {                       // NV12: Y plane [h,w], then the interleaved UV plane [h/2,w]
          const long long luma = off + (long long)sx0 + k;
          const long long chroma = kSurf ? sf.uv_off + (long long)sx0 + k : luma + (long long)h * w;
          const long long pitch = kSurf ? sf.pitch : (long long)w, uv_pitch = kSurf ? sf.uv_pitch : (long long)w;
          auto rows = [&](auto wide) {
            for (int sy = sy0; sy < sy1; ++sy) {
              unsigned y[2], uv[2];
              load_bytes<8, decltype(wide)::value>(src, luma + sy * pitch, src_bytes, y);
              load_bytes<8, decltype(wide)::value>(src, chroma + (sy >> 1) * uv_pitch, src_bytes, uv);
#pragma unroll
              for (int p = 0; p < 4; ++p) {
                const unsigned c = (uv[p >> 1] >> (16 * (p & 1))) & 0xffffu, yy = (y[p >> 1] >> (16 * (p & 1))) & 0xffffu;
                add(2 * p, yy & 255u, c & 255u, c >> 8);
                add(2 * p + 1, yy >> 8, c & 255u, c >> 8);
              }
            }
          };
          // (the luma plane of a dense frame lies in front of its chroma plane; a surface's planes lie anywhere)
          if ((!kSurf || luma + (sy1 - 1) * pitch + 8 <= src_bytes) && chroma + ((sy1 - 1) >> 1) * uv_pitch + 8 <= src_bytes)
            rows(std::true_type{});
          else
            rows(std::false_type{});
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          cs[k + j] = acc[j];
          cs[kAreaYuvPix + k + j] = acc[8 + j];
          cs[2 * kAreaYuvPix + k + j] = acc[16 + j];
        }
      }
    }
    __syncthreads();
    // horizontal half: output ox of channel c adds its window's picture columns and divides once; (q, r) of ox P / S is
    // passed along a run of outputs
    auto pixel = [&](int c, int& q, int& r) -> float {
      int q1 = q + qs, r1 = r + rs;   // (ox + 1) P = q1 S + r1
      if (r1 >= S) r1 -= S, ++q1;
      const int ax = q, bx = q1 + (r1 > 0);
      q = q1, r = r1;
      const int ua = flip ? P - bx : ax, ub = flip ? P - ax : bx;
      const int xa = ua - pad_left > 0 ? ua - pad_left : 0;
      const int xb = ub - pad_left < w ? ub - pad_left : w;
      int sum = 0;
      if (any) {
        const int step = yuv ? 1 : 3, first = yuv ? c * kAreaYuvPix : cfirst + cstep * c;
        for (int x = xa; x < xb; ++x) sum += cs[first + step * (x - sx0)];
      }
      return (float)sum / (float)(255 * ((by - ay) * (bx - ax)));
    };
    const int nout = ox1 - ox0;
    if ((S & 3) == 0) {   // ox0 and nout are multiples of 4
      const int nq = nout >> 2;
      for (int i = t; i < 3 * nq; i += 256) {
        const int c = i / nq, ox = ox0 + 4 * (i - c * nq);
        int q, r;
        divmod(ox, q, r);
        float4 v;
        v.x = pixel(c, q, r);
        v.y = pixel(c, q, r);
        v.z = pixel(c, q, r);
        v.w = pixel(c, q, r);
        *reinterpret_cast<float4*>(out + (size_t)c * total + ox) = v;
      }
    } else {
      for (int i = t; i < 3 * nout; i += 256) {
        const int c = i / nout, ox = ox0 + (i - c * nout);
        int q, r;
        divmod(ox, q, r);
        out[(size_t)c * total + ox] = pixel(c, q, r);
      }
    }
    __syncthreads();   // the next segment overwrites cs
  }
}

// ---- radar heat map ------------------------------------------------------------------------------------------
constexpr int HM_MAX = 64;  // max bins per side (radar_maps_size is 32 in the reference)

// bin index of np.histogramdd: searchsorted(edges, v, side="right") - 1 with edges = linspace(0, hi, nb + 1)
// (edge i = i * step in float64, last edge = hi exactly); v == hi belongs to the last bin; -1 = outside.
__device__ inline int hist_bin(double v, double hi, int nb) {
  if (!(v >= 0.0) || !(v <= hi)) return -1;
  if (v == hi) return nb - 1;
  const double step = hi / (double)nb;
  int b = (int)(v / step);
  if (b > nb - 1) b = nb - 1;
  // make b the largest i with edge_i <= v (the division can be off by one ulp either way)
  while (b > 0 && (double)b * step > v) --b;
  while (b + 1 < nb && (double)(b + 1) * step <= v) ++b;
  return b;
}

struct HeatP {
  const double* points;   // [total, 4] = (u, v, depth, velocity) rows, frames concatenated
  const int* offsets;     // [n + 1] row range of frame i
  const int* sizes;       // [n, 2] = (w, h) of the original image
  float* out;             // [n, 3, ms, ms]
  int maps_size;          // radar_maps_size (32)
  int ms;                 // output side (img_size / 16); kRect: the output height mh
  int mw, a, b;           // kRect only: the output width, a = mh / gcd(mh, mw), b = mw / gcd(mh, mw)
};

// kRect = false: me_radar_heatmap_f32.  kRect = true: me_radar_heatmap_rect_f32 - the same bins, padded to the smallest
// (a k) x (b k) that holds them (letterbox_geom) and resized to mh x mw with one factor per axis.
template <bool kRect>
__global__ __launch_bounds__(256) void radar_heatmap_kernel(HeatP p) {
  __shared__ float maps[3][HM_MAX * HM_MAX];  // [c][y * bw + x], already float32 (ToTensor().float())
  const int f = blockIdx.x;
  const int img_w = p.sizes[2 * f], img_h = p.sizes[2 * f + 1];
  const int r0 = p.offsets[f], npts = p.offsets[f + 1] - r0;
  // scale = max(img_size) / radar_maps_size; bin_w, bin_h = round(w / scale), round(h / scale): python round =
  // round-half-even on the float64 quotient
  const double scale = (double)(img_w > img_h ? img_w : img_h) / (double)p.maps_size;
  const int bw = (int)rint((double)img_w / scale), bh = (int)rint((double)img_h / scale);
  const int nbins = bw * bh;
  // one thread per bin walks the points in order: the weighted sums are the sequential float64 sums np.bincount makes
  for (int b = threadIdx.x; b < nbins; b += 256) {
    const int by = b / bw, bx = b - by * bw;
    double cnt = 0.0, sd = 0.0, sv = 0.0;
    for (int i = 0; i < npts; ++i) {
      const double* q = p.points + (size_t)(r0 + i) * 4;
      const int ix = hist_bin(q[0], (double)img_w, bw);
      const int iy = hist_bin(q[1], (double)img_h, bh);
      if (ix == bx && iy == by) {
        cnt += 1.0;
        sd += q[2];
        sv += q[3];
      }
    }
    double h1 = sd / (cnt + 1e-6);          // mean depth per bin
    h1 = h1 < 1.0 ? 100.0 : h1;             // empty / too close -> far away
    const double h2 = fabs(sv / (cnt + 1e-6));
    // ranges ((0,5), (12,0), (0,4)) then clip to [0,1]
    double c0 = (cnt - 0.0) / (5.0 - 0.0), c1 = (h1 - 12.0) / (0.0 - 12.0), c2 = (h2 - 0.0) / (4.0 - 0.0);
    c0 = fmin(fmax(c0, 0.0), 1.0);
    c1 = fmin(fmax(c1, 0.0), 1.0);
    c2 = fmin(fmax(c2, 0.0), 1.0);
    maps[0][b] = (float)c0;
    maps[1][b] = (float)c1;
    maps[2][b] = (float)c2;
  }
  __syncthreads();
  if constexpr (kRect) {
    // bh, bw <= HM_MAX and the entry point refuses a * HM_MAX or b * HM_MAX above 2^30: Ph, Pw <= 2^30, geo.ok holds
    const LetterboxGeom geo = letterbox_geom(bh, bw, p.a, p.b);
    const int Ph = geo.Ph, Pw = geo.Pw, pad_top = geo.top, pad_left = geo.left, mh = p.ms, mw = p.mw;
    const float rs_y = mh > 1 ? (float)(Ph - 1) / (float)(mh - 1) : 0.f;
    const float rs_x = mw > 1 ? (float)(Pw - 1) / (float)(mw - 1) : 0.f;
    auto at = [&](int c, int y, int x) -> float {
      const int sy = y - pad_top, sx = x - pad_left;
      return ((unsigned)sy < (unsigned)bh && (unsigned)sx < (unsigned)bw) ? maps[c][sy * bw + sx] : 0.f;
    };
    float* out = p.out + (size_t)f * 3 * mh * mw;
    for (int idx = threadIdx.x; idx < 3 * mh * mw; idx += 256) {
      const int c = idx / (mh * mw), rem = idx - c * mh * mw;
      const int oy = rem / mw, ox = rem - oy * mw;
      float v;
      if (Ph == mh && Pw == mw) {
        v = at(c, oy, ox);
      } else {
        const float h1r = rs_y * (float)oy, w1r = rs_x * (float)ox;
        const int h1 = (int)h1r, w1 = (int)w1r;
        const int h1p = h1 < Ph - 1 ? 1 : 0, w1p = w1 < Pw - 1 ? 1 : 0;
        const float h1l = h1r - (float)h1, w1l = w1r - (float)w1;
        const float h0l = 1.f - h1l, w0l = 1.f - w1l;
        v = h0l * (w0l * at(c, h1, w1) + w1l * at(c, h1, w1 + w1p)) +
            h1l * (w0l * at(c, h1 + h1p, w1) + w1l * at(c, h1 + h1p, w1 + w1p));
      }
      out[idx] = v;
    }
    return;
  }
  // pad_to_square (zeros) + bilinear, align_corners=True (aten upsample_bilinear2d, float32 arithmetic)
  const int P = bh > bw ? bh : bw;
  const int diff = bh > bw ? bh - bw : bw - bh;
  const int pad1 = diff / 2;
  const int pad_top = bh <= bw ? pad1 : 0, pad_left = bh <= bw ? 0 : pad1;
  const int ms = p.ms;
  const float rs = ms > 1 ? (float)(P - 1) / (float)(ms - 1) : 0.f;
  auto at = [&](int c, int y, int x) -> float {
    const int sy = y - pad_top, sx = x - pad_left;
    return ((unsigned)sy < (unsigned)bh && (unsigned)sx < (unsigned)bw) ? maps[c][sy * bw + sx] : 0.f;
  };
  float* out = p.out + (size_t)f * 3 * ms * ms;
  for (int idx = threadIdx.x; idx < 3 * ms * ms; idx += 256) {
    const int c = idx / (ms * ms), rem = idx - c * ms * ms;
    const int oy = rem / ms, ox = rem - oy * ms;
    float v;
    if (P == ms) {
      v = at(c, oy, ox);
    } else {
      const float h1r = rs * (float)oy, w1r = rs * (float)ox;
      const int h1 = (int)h1r, w1 = (int)w1r;
      const int h1p = h1 < P - 1 ? 1 : 0, w1p = w1 < P - 1 ? 1 : 0;
      const float h1l = h1r - (float)h1, w1l = w1r - (float)w1;
      const float h0l = 1.f - h1l, w0l = 1.f - w1l;
      v = h0l * (w0l * at(c, h1, w1) + w1l * at(c, h1, w1 + w1p)) +
          h1l * (w0l * at(c, h1 + h1p, w1) + w1l * at(c, h1 + h1p, w1 + w1p));
    }
    out[idx] = v;
  }
}

}  // namespace

extern "C" {

int me_image_pad_resize_u8_f32(const uint8_t* src, int32_t h, int32_t w, float* dst, int32_t size, void* stream) {
  ME_REQUIRE(src && dst, ME_E_NULLPTR, "me_image_pad_resize_u8_f32: null pointer");
  ME_REQUIRE(h > 0 && w > 0 && size > 0, ME_E_BADARG, "me_image_pad_resize_u8_f32: non-positive size");
  ME_REQUIRE((long long)size * size < (1ll << 30), ME_E_TOOBIG, "me_image_pad_resize_u8_f32: output too large");
  int blocks = (int)me::ceil_div((int64_t)size * size, 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(image_pad_resize_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, h, w, dst, size, 0);
  return me::check_launch("image_pad_resize_kernel");
}

int me_image_pad_resize_flip_u8_f32(const uint8_t* src, int32_t h, int32_t w, float* dst, int32_t size, int32_t flip,
                                    void* stream) {
  ME_REQUIRE(src && dst, ME_E_NULLPTR, "me_image_pad_resize_flip_u8_f32: null pointer");
  ME_REQUIRE(h > 0 && w > 0 && size > 0, ME_E_BADARG, "me_image_pad_resize_flip_u8_f32: non-positive size");
  ME_REQUIRE((long long)size * size < (1ll << 30), ME_E_TOOBIG, "me_image_pad_resize_flip_u8_f32: output too large");
  int blocks = (int)me::ceil_div((int64_t)size * size, 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(image_pad_resize_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, h, w, dst, size,
                     flip ? 1 : 0);
  return me::check_launch("image_pad_resize_kernel");
}

int me_image_batch_pad_resize_flip_u8_f32(const uint8_t* src, int64_t src_bytes, const int64_t* desc, int32_t n,
                                          float* dst, int32_t size, void* stream) {
  if (n == 0) return 0;
  ME_REQUIRE(src && desc && dst, ME_E_NULLPTR, "me_image_batch_pad_resize_flip_u8_f32: null pointer");
  ME_REQUIRE(n > 0 && n <= 65535 && size > 0 && src_bytes > 0, ME_E_BADARG,
             "me_image_batch_pad_resize_flip_u8_f32: bad n / size / src_bytes");
  ME_REQUIRE((long long)size * size < (1ll << 30), ME_E_TOOBIG, "me_image_batch_pad_resize_flip_u8_f32: output too large");
  ME_REQUIRE((size & 3) != 0 || me::aligned16(dst), ME_E_ALIGN, "me_image_batch_pad_resize_flip_u8_f32: dst not 16-byte aligned");
  const int per_block = (size & 3) == 0 ? kBatchPix : 256;
  int tiles = (int)me::ceil_div((int64_t)size * size, per_block);
  if (tiles > 1024) tiles = 1024;
  hipLaunchKernelGGL(image_batch_pad_resize_kernel, dim3(tiles, n), dim3(256), 0, (hipStream_t)stream, src,
                     (long long)src_bytes, reinterpret_cast<const long long*>(desc), dst, size);
  return me::check_launch("image_batch_pad_resize_kernel");
}

int me_image_batch_formats_u8_f32(const uint8_t* src, int64_t src_bytes, const int64_t* desc, int32_t n, float* dst,
                                  int32_t size, void* stream) {
  if (n == 0) return 0;
  ME_REQUIRE(src && desc && dst, ME_E_NULLPTR, "me_image_batch_formats_u8_f32: null pointer");
  ME_REQUIRE(n > 0 && n <= 65535 && size > 0 && src_bytes > 0, ME_E_BADARG,
             "me_image_batch_formats_u8_f32: bad n / size / src_bytes");
  ME_REQUIRE((long long)size * size < (1ll << 30), ME_E_TOOBIG, "me_image_batch_formats_u8_f32: output too large");
  ME_REQUIRE((size & 3) != 0 || me::aligned16(dst), ME_E_ALIGN, "me_image_batch_formats_u8_f32: dst not 16-byte aligned");
  const int per_block = (size & 3) == 0 ? kBatchPix : 256;
  int tiles = (int)me::ceil_div((int64_t)size * size, per_block);
  if (tiles > 1024) tiles = 1024;
  hipLaunchKernelGGL(image_batch_formats_kernel, dim3(tiles, n), dim3(256), 0, (hipStream_t)stream, src,
                     (long long)src_bytes, reinterpret_cast<const long long*>(desc), dst, size);
  return me::check_launch("image_batch_formats_kernel");
}

int me_image_batch_letterbox_u8_f32(const uint8_t* src, int64_t src_bytes, const int64_t* desc, int32_t n, float* dst,
                                    int32_t height, int32_t width, void* stream) {
  if (n == 0) return 0;
  ME_REQUIRE(src && desc && dst, ME_E_NULLPTR, "me_image_batch_letterbox_u8_f32: null pointer");
  ME_REQUIRE(n > 0 && n <= 65535 && height > 0 && width > 0 && src_bytes > 0, ME_E_BADARG,
             "me_image_batch_letterbox_u8_f32: bad n / height / width / src_bytes");
  ME_REQUIRE((long long)height * width < (1ll << 30), ME_E_TOOBIG, "me_image_batch_letterbox_u8_f32: output too large");
  ME_REQUIRE((width & 3) != 0 || me::aligned16(dst), ME_E_ALIGN, "me_image_batch_letterbox_u8_f32: dst not 16-byte aligned");
  const int per_block = (width & 3) == 0 ? kBatchPix : 256;
  int tiles = (int)me::ceil_div((int64_t)height * width, per_block);
  if (tiles > 1024) tiles = 1024;
  const int g = me::gcd_i32(height, width);
  hipLaunchKernelGGL(image_batch_letterbox_kernel<false>, dim3(tiles, n), dim3(256), 0, (hipStream_t)stream, src,
                     (long long)src_bytes, reinterpret_cast<const long long*>(desc), dst, height, width, height / g, width / g);
  return me::check_launch("image_batch_letterbox_kernel");
}

int me_image_batch_area_u8_f32(const uint8_t* src, int64_t src_bytes, const int64_t* desc, int32_t n, float* dst,
                               int32_t size, void* stream) {
  if (n == 0) return 0;
  ME_REQUIRE(src && desc && dst, ME_E_NULLPTR, "me_image_batch_area_u8_f32: null pointer");
  ME_REQUIRE(n > 0 && n <= 65535 && size > 0 && src_bytes > 0, ME_E_BADARG,
             "me_image_batch_area_u8_f32: bad n / size / src_bytes");
  ME_REQUIRE((long long)size * size < (1ll << 30), ME_E_TOOBIG, "me_image_batch_area_u8_f32: output too large");
  ME_REQUIRE((size & 3) != 0 || me::aligned16(dst), ME_E_ALIGN, "me_image_batch_area_u8_f32: dst not 16-byte aligned");
  hipLaunchKernelGGL(image_batch_area_kernel<false>, dim3(size, n), dim3(256), 0, (hipStream_t)stream, src, (long long)src_bytes,
                     reinterpret_cast<const long long*>(desc), dst, size);
  return me::check_launch("image_batch_area_kernel");
}

int me_image_batch_surfaces_u8_f32(const int64_t* desc, int32_t n, float* dst, int32_t height, int32_t width, int32_t resize,
                                   void* stream) {
  if (n == 0) return 0;
  ME_REQUIRE(desc && dst, ME_E_NULLPTR, "me_image_batch_surfaces_u8_f32: null pointer");
  ME_REQUIRE(n > 0 && n <= 65535 && height > 0 && width > 0, ME_E_BADARG, "me_image_batch_surfaces_u8_f32: bad n / height / width");
  ME_REQUIRE(resize == 0 || resize == 1, ME_E_BADARG, "me_image_batch_surfaces_u8_f32: resize %d is neither 0 (nearest) nor 1 (area)",
             resize);
  ME_REQUIRE(resize == 0 || height == width, ME_E_BADARG,
             "me_image_batch_surfaces_u8_f32: the area resize has no rectangular form (%d x %d)", height, width);
  ME_REQUIRE((long long)height * width < (1ll << 30), ME_E_TOOBIG, "me_image_batch_surfaces_u8_f32: output too large");
  ME_REQUIRE((width & 3) != 0 || me::aligned16(dst), ME_E_ALIGN, "me_image_batch_surfaces_u8_f32: dst not 16-byte aligned");
  const long long* d = reinterpret_cast<const long long*>(desc);
  if (resize == 1) {
    hipLaunchKernelGGL(image_batch_area_kernel<true>, dim3(height, n), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)nullptr, 0ll, d, dst, height);
    return me::check_launch("image_batch_area_kernel");
  }
  const int per_block = (width & 3) == 0 ? kBatchPix : 256;
  int tiles = (int)me::ceil_div((int64_t)height * width, per_block);
  if (tiles > 1024) tiles = 1024;
  const int g = me::gcd_i32(height, width);
  hipLaunchKernelGGL(image_batch_letterbox_kernel<true>, dim3(tiles, n), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)nullptr, 0ll, d, dst, height, width, height / g, width / g);
  return me::check_launch("image_batch_letterbox_kernel");
}

int me_radar_heatmap_f32(const double* points, const int32_t* offsets, const int32_t* sizes, int32_t n,
                         int32_t radar_maps_size, float* out, int32_t map_size, void* stream) {
  if (n == 0) return 0;
  ME_REQUIRE(points && offsets && sizes && out, ME_E_NULLPTR, "me_radar_heatmap_f32: null pointer");
  ME_REQUIRE(n > 0 && map_size > 0, ME_E_BADARG, "me_radar_heatmap_f32: bad n / map_size");
  ME_REQUIRE(radar_maps_size >= 1 && radar_maps_size <= HM_MAX, ME_E_BADARG,
             "me_radar_heatmap_f32: radar_maps_size %d outside [1, %d]", radar_maps_size, HM_MAX);
  HeatP p{points, offsets, sizes, out, radar_maps_size, map_size, 0, 0, 0};
  hipLaunchKernelGGL(radar_heatmap_kernel<false>, dim3(n), dim3(256), 0, (hipStream_t)stream, p);
  return me::check_launch("radar_heatmap_kernel");
}

int me_radar_heatmap_rect_f32(const double* points, const int32_t* offsets, const int32_t* sizes, int32_t n,
                              int32_t radar_maps_size, float* out, int32_t map_h, int32_t map_w, void* stream) {
  if (n == 0) return 0;
  ME_REQUIRE(points && offsets && sizes && out, ME_E_NULLPTR, "me_radar_heatmap_rect_f32: null pointer");
  ME_REQUIRE(n > 0 && map_h > 0 && map_w > 0, ME_E_BADARG, "me_radar_heatmap_rect_f32: bad n / map size %d x %d", map_h, map_w);
  ME_REQUIRE((long long)map_h * map_w < (1ll << 28), ME_E_TOOBIG, "me_radar_heatmap_rect_f32: map %d x %d too large", map_h, map_w);
  ME_REQUIRE(radar_maps_size >= 1 && radar_maps_size <= HM_MAX, ME_E_BADARG,
             "me_radar_heatmap_rect_f32: radar_maps_size %d outside [1, %d]", radar_maps_size, HM_MAX);
  const int g = me::gcd_i32(map_h, map_w);
  // the padded bin map is at most (a HM_MAX) x (b HM_MAX): keep it within the geometry's 2^30 (1 x 2^27 would not be)
  ME_REQUIRE((long long)(map_h / g) * HM_MAX <= (1ll << 30) && (long long)(map_w / g) * HM_MAX <= (1ll << 30), ME_E_TOOBIG,
             "me_radar_heatmap_rect_f32: the aspect ratio of %d x %d pads the bins beyond 2^30", map_h, map_w);
  HeatP p{points, offsets, sizes, out, radar_maps_size, map_h, map_w, map_h / g, map_w / g};
  hipLaunchKernelGGL(radar_heatmap_kernel<true>, dim3(n), dim3(256), 0, (hipStream_t)stream, p);
  return me::check_launch("radar_heatmap_kernel");
}

}  // extern "C"

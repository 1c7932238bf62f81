// Page compositing for the segmentation heads: the per-bubble predictions of one manga page pasted back into ONE
// page-sized BGR label map, what the reference's test_BE_manga.py:63-147 / :160-225 do on the host with full-page float tensors per
// bubble.  Integer and boolean arithmetic only: the result is the reference's, bit for bit.
//
// The page is walked as the flat array of its H*W pixels.  A lane owns four consecutive pixels = 12 bytes = three whole dwords whatever
// W is (a row start is dword-aligned only when W % 4 == 0; the flat group of four always is), a wave 256 pixels = 768 contiguous
// bytes, a workgroup 1024.  The descriptor table streams through LDS in chunks of DESC_CHUNK rows; every wave tests a row's box against
// its own pixel run ONCE (scalar, from LDS broadcasts) and only then do its lanes look at their pixels.  Bubbles claim pixels in
// table order, so a wave whose pixels are all claimed stops reading the table's boxes.  A wave that no box touches writes white with
// 16-byte stores (init) or nothing at all (continue).
#include "common.h"

namespace vp {
namespace {

constexpr int NT = 256;             // threads per workgroup
constexpr int PX = 4;               // pixels per lane
constexpr int DESC_CHUNK = 64;      // descriptor rows per LDS load (4 KB)
constexpr int RING = 6;             // (13 - 1) / 2: the reference dilates with a 13 x 13 kernel

// A descriptor row is four int4 (VP_BE_PAGE_DESC_INTS = 16 ints):
//   [0] anchor_x, anchor_y, bits of (float)SW / (float)size, bits of (float)SH / (float)size
//   [1] xmin, ymin, xmax, ymax          the box on the page, half-open
//   [2] rx0, ry0, rx1, ry1              kind 1: the content rectangle in crop coordinates, half-open
//   [3] label, kind, 0, 0
// kind 0: edge and content bits from the logits          kind 1: from the rectangle and its 6-pixel ring
// kind 2: from the page mask and its 13 x 13 window      kind 3: edge bit from the logits, content bit from the page mask

__device__ __forceinline__ int nearest(int j, float scale, int S) {
  // torch's nearest: min((int)floorf(j * scale), S - 1) in fp32; the scale comes rounded once from the host.  (The max keeps a read
  // inside its plane whatever the table holds; a validated table never gives a negative j.)
  return max(min((int)floorf((float)j * scale), S - 1), 0);
}

__global__ __launch_bounds__(NT) void be_compose_page_kernel(const float* __restrict__ edges, size_t edge_stride,
                                                              const float* __restrict__ masks, size_t mask_stride,
                                                              const int4* __restrict__ desc, int m,
                                                              const unsigned char* __restrict__ page_masks, unsigned char* __restrict__ page,
                                                              int H, int W, int SH, int SW, float threshold, int init_white, int wide_ok) {
  __shared__ int4 sdesc[DESC_CHUNK * 4];
  const int npix = H * W;                                        // (the entry point keeps H * W <= 2^30)
  const int lane = threadIdx.x & 63;
  const int wave_p0 = (blockIdx.x * NT + (threadIdx.x & ~63)) * PX;                    // this wave's pixel run [wave_p0, wave_p1]
  const bool wave_live = wave_p0 < npix;
  const int wave_p1 = min(wave_p0 + 64 * PX, npix) - 1;
  // the wave's bounding box on the page: one row -> its exact columns; more rows -> every column
  int wy0 = 0, wy1 = -1, wx0 = 0, wx1 = -1;
  if (wave_live) {
    wy0 = wave_p0 / W;
    wy1 = wave_p1 / W;
    wx0 = wy0 == wy1 ? wave_p0 - wy0 * W : 0;
    wx1 = wy0 == wy1 ? wave_p1 - wy0 * W : W - 1;
  }
  wy0 = __builtin_amdgcn_readfirstlane(wy0);
  wy1 = __builtin_amdgcn_readfirstlane(wy1);
  wx0 = __builtin_amdgcn_readfirstlane(wx0);
  wx1 = __builtin_amdgcn_readfirstlane(wx1);

  const int p0 = wave_p0 + lane * PX;                            // this lane's first pixel
  const int nvalid = max(0, min(PX, npix - p0));
  int py[PX], px[PX];
  {
    int y = p0 < npix ? p0 / W : 0, x = p0 < npix ? p0 - y * W : 0;
#pragma unroll
    for (int p = 0; p < PX; ++p) {
      py[p] = y;
      px[p] = x;
      if (++x == W) { x = 0; ++y; }
    }
  }
  unsigned char* dst = page + (size_t)p0 * 3;
  unsigned rgb[PX];                                              // byte 0 edge, byte 1 label, byte 2 content
  bool open[PX];                                                 // still white and on the page
#pragma unroll
  for (int p = 0; p < PX; ++p) {
    rgb[p] = 0xffffffu;
    open[p] = p < nvalid;
  }
  if (!init_white && nvalid > 0) {                               // continue a page: a pixel that is not white is claimed
    if (nvalid == PX) {
      const unsigned* d = reinterpret_cast<const unsigned*>(dst);
      const unsigned d0 = d[0], d1 = d[1], d2 = d[2];
      rgb[0] = d0 & 0xffffffu;
      rgb[1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
      rgb[2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
      rgb[3] = d2 >> 8;
    } else {
      for (int p = 0; p < nvalid; ++p)
        rgb[p] = (unsigned)dst[3 * p] | ((unsigned)dst[3 * p + 1] << 8) | ((unsigned)dst[3 * p + 2] << 16);
    }
#pragma unroll
    for (int p = 0; p < PX; ++p) open[p] = p < nvalid && rgb[p] == 0xffffffu;
  }
  bool touched = false;                                          // a box met this wave's run (wave-uniform)
  bool wave_open = wave_live && __any(open[0] | open[1] | open[2] | open[3]);

  for (int c0 = 0; c0 < m; c0 += DESC_CHUNK) {
    const int rows = min(DESC_CHUNK, m - c0);
    __syncthreads();
    for (int i = threadIdx.x; i < rows * 4; i += NT) sdesc[i] = desc[(size_t)c0 * 4 + i];
    __syncthreads();
    if (!wave_open) continue;                                    // (the barriers above are still met by every wave)
    for (int r = 0; r < rows; ++r) {
      const int4 box = sdesc[r * 4 + 1];
      const int xmin = __builtin_amdgcn_readfirstlane(box.x), ymin = __builtin_amdgcn_readfirstlane(box.y);
      const int xmax = __builtin_amdgcn_readfirstlane(box.z), ymax = __builtin_amdgcn_readfirstlane(box.w);
      if (xmax <= wx0 || xmin > wx1 || ymax <= wy0 || ymin > wy1) continue;            // culled for the whole wave
      touched = true;
      const int4 a = sdesc[r * 4 + 0], rect = sdesc[r * 4 + 2], lk = sdesc[r * 4 + 3];
      const int kind = __builtin_amdgcn_readfirstlane(lk.y);
      const unsigned label = (unsigned)lk.x & 0xffu;
      const float sx = __int_as_float(a.z), sy = __int_as_float(a.w);
      const size_t bubble = (size_t)(c0 + r);
      const float* e_img = edges + bubble * edge_stride;
      const float* m_img = masks + bubble * mask_stride;
      const unsigned char* pm = page_masks + bubble * (size_t)npix;
#pragma unroll
      for (int p = 0; p < PX; ++p) {
        const int y = py[p], x = px[p];
        if (!open[p] || x < xmin || x >= xmax || y < ymin || y >= ymax) continue;
        const int cy = a.y + y - ymin, cx = a.x + x - xmin;
        bool E, M;
        if (kind == 0 || kind == 3) {
          const size_t at = (size_t)nearest(cy, sy, SH) * SW + nearest(cx, sx, SW);
          E = !(e_img[at] < threshold);                          // a NaN counts as set, as in the reference
          M = kind == 0 ? !(m_img[at] < threshold) : pm[(size_t)y * W + x] != 0;
        } else if (kind == 1) {
          M = cx >= rect.x && cx < rect.z && cy >= rect.y && cy < rect.w;
          E = rect.x < rect.z && rect.y < rect.w && cx >= rect.x - RING && cx < rect.z + RING && cy >= rect.y - RING && cy < rect.w + RING;
        } else {
          M = pm[(size_t)y * W + x] != 0;
          E = false;
          if (!M) {                                              // the 13 x 13 window, restricted to the box (the reference convolves the crop)
            const int y0 = max(y - RING, max(ymin, 0)), y1 = min(y + RING, min(ymax, H) - 1);
            const int x0 = max(x - RING, max(xmin, 0)), x1 = min(x + RING, min(xmax, W) - 1);
            unsigned any = 0;
            for (int yy = y0; yy <= y1; ++yy)
              for (int xx = x0; xx <= x1; ++xx) any |= pm[(size_t)yy * W + xx];
            E = any != 0;
          }
        }
        E = E && !M;
        if (E | M) {
          open[p] = false;
          rgb[p] = E ? (0xffu | (label << 8)) : ((label << 8) | 0xff0000u);
        }
      }
      wave_open = __any(open[0] | open[1] | open[2] | open[3]);
      if (!wave_open) break;
    }
  }
  if (!wave_live) return;
  if (!touched) {                                                // no box met this wave
    if (!init_white) return;                                     // continue: the page stays as it is
    if (wide_ok && wave_p1 - wave_p0 + 1 == 64 * PX) {           // a full run of 768 bytes on a 16-byte boundary: 48 lanes x 16 bytes
      if (lane < 48) reinterpret_cast<uint4*>(page + (size_t)wave_p0 * 3)[lane] = make_uint4(~0u, ~0u, ~0u, ~0u);
      return;
    }
  }
  if (nvalid == PX) {                                            // four pixels = three dwords
    unsigned* d = reinterpret_cast<unsigned*>(dst);
    d[0] = rgb[0] | (rgb[1] << 24);
    d[1] = (rgb[1] >> 8) | (rgb[2] << 16);
    d[2] = (rgb[2] >> 16) | (rgb[3] << 8);
  } else {
    for (int p = 0; p < nvalid; ++p) {                           // the page's last one to three pixels
      dst[3 * p] = (unsigned char)rgb[p];
      dst[3 * p + 1] = (unsigned char)(rgb[p] >> 8);
      dst[3 * p + 2] = (unsigned char)(rgb[p] >> 16);
    }
  }
}

}  // namespace
}  // namespace vp

using namespace vp;

extern "C" {

int vp_be_compose_page_u8(const float* edges, size_t edge_stride, const float* masks, size_t mask_stride, const int* desc, int m,
                          const unsigned char* page_masks, unsigned char* page, int H, int W, int SH, int SW, float threshold,
                          int init_white, vp_stream stream) {
  VP_REQUIRE(page, "vp_be_compose_page_u8: null page");
  VP_REQUIRE(H > 0 && W > 0 && (long long)H * W <= (1LL << 30), "vp_be_compose_page_u8: the page must have 1 .. 2^30 pixels");
  VP_REQUIRE(m >= 0 && SH > 0 && SW > 0, "vp_be_compose_page_u8: m must not be negative, the logit planes not empty");
  VP_REQUIRE(m == 0 || desc, "vp_be_compose_page_u8: null descriptor table");
  VP_REQUIRE(((uintptr_t)desc & 15) == 0 && ((uintptr_t)page & 3) == 0 && ((uintptr_t)edges & 3) == 0 && ((uintptr_t)masks & 3) == 0,
             "vp_be_compose_page_u8: the table must be 16-byte aligned, the page and the logits 4-byte aligned");
  if (m == 0 && !init_white) return VP_OK;                       // nothing to add to the page
  const int npix = H * W;
  const unsigned grid = (unsigned)((npix + NT * PX - 1) / (NT * PX));
  hipLaunchKernelGGL(be_compose_page_kernel, dim3(grid), dim3(NT), 0, (hipStream_t)stream, edges, edge_stride, masks, mask_stride,
                     reinterpret_cast<const int4*>(desc), m, page_masks, page, H, W, SH, SW, threshold, init_white,
                     (int)(((uintptr_t)page & 15) == 0));
  return check_launch("vp_be_compose_page_u8");
}

}  // extern "C"

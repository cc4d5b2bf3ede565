// On-device loader augmentation: the Pillow / torchvision pipelines of the reference's augment_zoo
// (semi_seg/augment.py:36-283, applied by contrastyou/augment/synchronize.py:76-165) from a store of uint8 slices that
// stays in device memory.  include/contrastyou_hip.h states the record of a view and the arithmetic, DESIGN.md
// section 3 where it comes from in Pillow.  Two launches per batch: the geometry of every image and label view, then
// the jitter and ToTensor of the image views.  The parameters are drawn on the host: no sin, cos or division here.
#include "cy_common.h"

namespace {

struct AugView {
  const uint8_t* src;  // the slice in the arena this thread reads (image or label)
  int H, W;            // its size
  const int32_t* ip;
};

// canvas pixel (y, x), inside the canvas: the source through the pre-window, 0 where the window leaves the source
__device__ __forceinline__ int aug_canvas(const AugView& v, int y, int x) {
  const int sy = y + v.ip[CY_AUG_IP_PY], sx = x + v.ip[CY_AUG_IP_PX];
  if (sy < 0 || sy >= v.H || sx < 0 || sx >= v.W) return 0;
  return v.src[(size_t)sy * v.W + sx];
}

__device__ __forceinline__ int aug_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Pillow's affine_fixed (Geometry.c), nearest: integers only
__device__ __forceinline__ int aug_rotate_nearest(const AugView& v, int y, int x, int ch, int cw) {
  const int32_t* a = v.ip + CY_AUG_IP_A0;
  const long long xin = ((long long)a[2] + (long long)y * a[1] + (long long)x * a[0]) >> 16;
  const long long yin = ((long long)a[5] + (long long)y * a[4] + (long long)x * a[3]) >> 16;
  if (xin < 0 || xin >= cw || yin < 0 || yin >= ch) return 0;
  return aug_canvas(v, (int)yin, (int)xin);
}

// Pillow's affine_transform + bilinear_filter8 (Geometry.c): f64, every product and sum rounded on its own as the C
// compiler of Pillow's build and NumPy round them -- hipcc would contract them to fma
#pragma clang fp contract(off)
__device__ __forceinline__ int aug_rotate_bilinear(const AugView& v, const double* __restrict__ m, int y, int x, int ch,
                                                   int cw) {
  const double xc = (double)x + 0.5, yc = (double)y + 0.5;
  double xin = m[0] * xc + m[1] * yc + m[2];
  double yin = m[3] * xc + m[4] * yc + m[5];
  if (xin < 0.0 || xin >= (double)cw || yin < 0.0 || yin >= (double)ch) return 0;
  xin -= 0.5, yin -= 0.5;
  const double fx = floor(xin), fy = floor(yin);
  const int x0 = (int)fx, y0 = (int)fy;
  const double dx = xin - fx, dy = yin - fy;
  const int xa = aug_clamp(x0, cw - 1), xb = aug_clamp(x0 + 1, cw - 1), ya = aug_clamp(y0, ch - 1);
  const int p = aug_canvas(v, ya, xa), q = aug_canvas(v, ya, xb);
  const double v1 = (double)p + (double)(q - p) * dx;
  double v2 = v1;
  if (y0 + 1 >= 0 && y0 + 1 < ch) {
    const int r = aug_canvas(v, y0 + 1, xa), s = aug_canvas(v, y0 + 1, xb);
    v2 = (double)r + (double)(s - r) * dx;
  }
  return (int)(uint8_t)(int)(v1 + (v2 - v1) * dy);  // in 0..255: a convex mix of pixel values, truncated
}

// stage A.  blockIdx.x: tile of CY_AUG_GEO_BLOCK output pixels, blockIdx.y: view, blockIdx.z: 0 image, 1 label
__global__ void __launch_bounds__(CY_AUG_GEO_BLOCK)
    aug_geometry_kernel(const uint8_t* __restrict__ store_img, const uint8_t* __restrict__ store_lab,
                        const int32_t* __restrict__ ip, const double* __restrict__ fp, int out_h, int out_w,
                        const uint8_t* __restrict__ label_lut, uint8_t* __restrict__ scratch,
                        int64_t* __restrict__ labels) {
  const int hw = out_h * out_w;
  const int i = blockIdx.x * CY_AUG_GEO_BLOCK + threadIdx.x;
  if (i >= hw) return;
  const int view = blockIdx.y;
  const bool is_label = blockIdx.z == 1;
  AugView v;
  v.ip = ip + (size_t)view * CY_AUG_IP_LEN;
  // the slice's table row travels in the record, which the host checked against its table before the launch
  const size_t off = (size_t)(uint32_t)v.ip[CY_AUG_IP_OFF_LO] | ((size_t)(uint32_t)v.ip[CY_AUG_IP_OFF_HI] << 32);
  v.src = (is_label ? store_lab : store_img) + off;
  v.H = v.ip[CY_AUG_IP_SRC_H], v.W = v.ip[CY_AUG_IP_SRC_W];
  const int ch = v.ip[CY_AUG_IP_CH], cw = v.ip[CY_AUG_IP_CW];
  int y = i / out_w + v.ip[CY_AUG_IP_QY], x = i % out_w + v.ip[CY_AUG_IP_QX];
  int val = 0;
  if (y >= 0 && y < ch && x >= 0 && x < cw) {
    if (v.ip[CY_AUG_IP_FLIPV]) y = ch - 1 - y;
    if (v.ip[CY_AUG_IP_FLIPH]) x = cw - 1 - x;
    if (!v.ip[CY_AUG_IP_ROT])
      val = aug_canvas(v, y, x);
    else if (is_label)
      val = aug_rotate_nearest(v, y, x, ch, cw);
    else
      val = aug_rotate_bilinear(v, fp + (size_t)view * CY_AUG_FP_LEN + CY_AUG_FP_M0, y, x, ch, cw);
  }
  const size_t o = (size_t)view * hw + i;
  if (is_label)
    labels[o] = (int64_t)label_lut[val];
  else
    scratch[o] = (uint8_t)val;
}

// ImageEnhance.Brightness / .Contrast on one value (Image.blend -> ImagingBlend: f32, truncation, clip)
__device__ __forceinline__ int aug_blend(float base, float f, int t) {
  const float r = base + f * ((float)t - base);  // contraction is off: product and sum rounded separately
  return r <= 0.f ? 0 : (r >= 255.f ? 255 : (int)r);
}

// exact sum of an unsigned per-thread value over the block of CY_AUG_JIT_BLOCK threads, in every thread
__device__ __forceinline__ unsigned aug_block_sum(unsigned v, unsigned* sh /* [CY_AUG_JIT_BLOCK / CY_WAVE] */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, CY_WAVE);
  __syncthreads();
  if ((threadIdx.x & (CY_WAVE - 1)) == 0) sh[threadIdx.x / CY_WAVE] = v;
  __syncthreads();
  unsigned s = 0;
#pragma unroll
  for (int w = 0; w < CY_AUG_JIT_BLOCK / CY_WAVE; ++w) s += sh[w];
  return s;
}

// stage B.  One block per view.  `map` is the composition of the view's jitter steps on 0..255; a contrast step needs
// the mean of the image as it stands, which is the sum of map[pixel] over the untouched scratch.
__global__ void __launch_bounds__(CY_AUG_JIT_BLOCK)
    aug_jitter_kernel(const uint8_t* __restrict__ scratch, const int32_t* __restrict__ ip,
                      const double* __restrict__ fp, int hw, const float* __restrict__ tensor_lut,
                      float* __restrict__ images) {
  __shared__ uint8_t map[256];
  __shared__ float out_lut[256];
  __shared__ unsigned wave_sums[CY_AUG_JIT_BLOCK / CY_WAVE];
  const int view = blockIdx.x, tid = threadIdx.x;
  const int32_t* vip = ip + (size_t)view * CY_AUG_IP_LEN;
  const double* vfp = fp + (size_t)view * CY_AUG_FP_LEN + CY_AUG_FP_F0;
  const uint8_t* src = scratch + (size_t)view * hw;
  if (tid < 256) map[tid] = (uint8_t)tid;
  int njit = vip[CY_AUG_IP_NJIT];
  njit = njit < 0 ? 0 : (njit > 3 ? 3 : njit);
  for (int k = 0; k < njit; ++k) {  // block-uniform
    const float f = (float)vfp[k];
    float base = 0.f;  // brightness blends with black
    if (vip[CY_AUG_IP_KIND0 + k] == CY_AUG_CONTRAST) {
      __syncthreads();  // map is complete
      unsigned part = 0;  // <= 255 * (512 * 512 / 1024) per thread, <= 255 * 512 * 512 in all: fits 32 bits
      for (int i = tid; i < hw; i += CY_AUG_JIT_BLOCK) part += map[src[i]];
      const unsigned long long sum = aug_block_sum(part, wave_sums);
      base = (float)(int)((2ull * sum + (unsigned)hw) / (2ull * (unsigned)hw));
    }
    __syncthreads();
    if (tid < 256) map[tid] = (uint8_t)aug_blend(base, f, map[tid]);  // each entry has one owner: no race
  }
  __syncthreads();
  if (tid < 256) out_lut[tid] = tensor_lut[map[tid]];
  __syncthreads();
  float* dst = images + (size_t)view * hw;
  for (int i = tid; i < hw; i += CY_AUG_JIT_BLOCK) dst[i] = out_lut[src[i]];
}

int aug_check_sizes(int views, int out_h, int out_w) {
  if (views < 1 || views > CY_AUG_MAX_VIEWS) return CY_ERR_SHAPE;
  if (out_h < 1 || out_h > CY_AUG_MAX_OUT || out_w < 1 || out_w > CY_AUG_MAX_OUT) return CY_ERR_SHAPE;
  return CY_OK;
}

bool aug_flag(int32_t v) { return v == 0 || v == 1; }
bool aug_offset(int32_t v) { return v >= -CY_AUG_MAX_OFFSET && v <= CY_AUG_MAX_OFFSET; }
bool aug_side(long long v) { return v >= 1 && v <= CY_AUG_MAX_SIDE; }

// the records of the views and the table rows they name, on the host copies
int aug_check_views(const int64_t* h_table, int slices, long long arena_bytes, const int32_t* h_ip, int views) {
  for (int v = 0; v < views; ++v) {
    const int32_t* p = h_ip + (size_t)v * CY_AUG_IP_LEN;
    const int32_t s = p[CY_AUG_IP_SLICE];
    if (s < 0 || s >= slices) return CY_ERR_SHAPE;
    const int64_t off = h_table[3 * (size_t)s], H = h_table[3 * (size_t)s + 1], W = h_table[3 * (size_t)s + 2];
    if (!aug_side(H) || !aug_side(W) || off < 0 || off > arena_bytes - H * W) return CY_ERR_SHAPE;
    if ((uint32_t)p[CY_AUG_IP_OFF_LO] != (uint32_t)(off & 0xffffffffLL) || p[CY_AUG_IP_OFF_HI] != (int32_t)(off >> 32) ||
        p[CY_AUG_IP_SRC_H] != H || p[CY_AUG_IP_SRC_W] != W)
      return CY_ERR_ARG;
    if (!aug_side(p[CY_AUG_IP_CH]) || !aug_side(p[CY_AUG_IP_CW])) return CY_ERR_SHAPE;
    if (!aug_offset(p[CY_AUG_IP_PY]) || !aug_offset(p[CY_AUG_IP_PX]) || !aug_offset(p[CY_AUG_IP_QY]) ||
        !aug_offset(p[CY_AUG_IP_QX]))
      return CY_ERR_SHAPE;
    if (!aug_flag(p[CY_AUG_IP_ROT]) || !aug_flag(p[CY_AUG_IP_FLIPV]) || !aug_flag(p[CY_AUG_IP_FLIPH]))
      return CY_ERR_ARG;
    const int32_t n = p[CY_AUG_IP_NJIT];
    if (n < 0 || n > 3) return CY_ERR_ARG;
    for (int k = 0; k < n; ++k)
      if (p[CY_AUG_IP_KIND0 + k] != CY_AUG_BRIGHTNESS && p[CY_AUG_IP_KIND0 + k] != CY_AUG_CONTRAST) return CY_ERR_ARG;
  }
  return CY_OK;
}

}  // namespace

extern "C" {

int cy_aug_plan(int views, int out_h, int out_w, cy_aug_plan_t* out) {
  if (!out) return CY_ERR_ARG;
  *out = {};
  const int rc = aug_check_sizes(views, out_h, out_w);
  out->status = rc;
  if (rc != CY_OK) return rc;
  const int hw = out_h * out_w;
  out->form = CY_AUG_FORM_TWO_STAGE;
  out->geo_grid_x = cy_cdiv(hw, CY_AUG_GEO_BLOCK);
  out->geo_grid_y = views;
  out->geo_grid_z = 2;
  out->jit_grid = views;
  out->jit_trips = cy_cdiv(hw, CY_AUG_JIT_BLOCK);
  out->jit_lds = 256 + 256 * 4 + (CY_AUG_JIT_BLOCK / CY_WAVE) * 4;
  out->scratch_bytes = views * hw;  // <= 4096 * 512 * 512 = 2^30
  out->launches = 2;
  return CY_OK;
}

int cy_aug_views(const uint8_t* store_img, const uint8_t* store_lab, const int64_t* h_table, int slices,
                 long long arena_bytes, const int32_t* ip, const int32_t* h_ip, const double* fp, int views, int out_h,
                 int out_w, const uint8_t* label_lut, const float* tensor_lut, float* images, int64_t* labels,
                 uint8_t* scratch, size_t scratch_bytes, void* stream) {
  if (!store_img || !h_table || !ip || !h_ip || !fp || !label_lut || !tensor_lut || !images || !scratch)
    return CY_ERR_ARG;
  if ((store_lab == nullptr) != (labels == nullptr)) return CY_ERR_ARG;
  int rc = aug_check_sizes(views, out_h, out_w);
  if (rc == CY_OK && slices < 1) rc = CY_ERR_SHAPE;
  if (rc == CY_OK) rc = aug_check_views(h_table, slices, arena_bytes, h_ip, views);
  if (rc != CY_OK) return rc;
  const int hw = out_h * out_w;
  if (scratch_bytes < (size_t)views * hw) return CY_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(cy_cdiv(hw, CY_AUG_GEO_BLOCK), views, labels ? 2 : 1);
  hipLaunchKernelGGL(aug_geometry_kernel, grid, dim3(CY_AUG_GEO_BLOCK), 0, st, store_img, store_lab, ip, fp,
                     out_h, out_w, label_lut, scratch, labels);
  hipLaunchKernelGGL(aug_jitter_kernel, dim3(views), dim3(CY_AUG_JIT_BLOCK), 0, st, (const uint8_t*)scratch, ip, fp,
                     hw, tensor_lut, images);
  CY_CHECK_LAUNCH();
  return CY_OK;
}

}  // extern "C"

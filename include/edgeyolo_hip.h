/*
 * edgeyolo_hip.h — C ABI of libedgeyolo_hip.so: the MI355X (gfx950) detection forward path of EdgeLine-YOLO.
 *
 * The reference (OneWalkman/EDGE-YOLO, an Ultralytics 8.3.63 fork) is pure Python/PyTorch and has NO FFI of its
 * own; the operators below are the ATen / torchvision call sites of its predict() hot path.
 * Each entry point names the reference function it replaces (paths relative to /root/reference/ultralytics/).
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory unless it says "host";
 *  - the caller owns all buffers; nothing is allocated, freed or synchronised inside; every launch goes to the
 *    hipStream_t passed as `stream` (so the calls can be captured into a hipGraph);
 *  - return 0 on success, a negative EY_E* code otherwise; ey_last_error() gives the message (thread local);
 *  - activations are NHWC ("channels last"): element (b,y,x,c) of a view lives at
 *        ptr + (((b*H + y)*W + x) * cstride + c)        [elements],
 *    so a channel slice of a wider tensor is just (ptr + c0, cstride = C_total): chunk/split/cat never copy;
 *  - dtype is the storage type of activations and packed weights (EY_F16 | EY_F32); accumulation, bias,
 *    softmax, decode and NMS arithmetic are always fp32.  EY_F32 is the parity mode (exact-f32 MFMA),
 *    EY_F16 the throughput mode.
 */
#ifndef EDGEYOLO_HIP_H
#define EDGEYOLO_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ey_stream_t; /* hipStream_t */

enum { EY_F16 = 0, EY_F32 = 1 };
enum { EY_ACT_NONE = 0, EY_ACT_SILU = 1, EY_ACT_RELU = 2, EY_ACT_SIGMOID = 3 };
enum { EY_OK = 0, EY_EINVAL = -1, EY_EUNSUPPORTED = -2, EY_ELAUNCH = -3 };

const char* ey_last_error(void);
int ey_version(void);
/* sizeof(ey_conv_desc) (which=0) / sizeof(ey_conv_direct_desc) (which=1) as compiled: lets a binding check its struct layout. */
size_t ey_abi_sizeof(int which);
/* Dispatch tunables (developer tools only; csrc/tune.h lists the names and the measured defaults).  They choose between kernels
 * that compute the same result -- thresholds such as "lean pointwise kernel below pw_m output pixels" -- never the arithmetic.
 * The library reads NO environment variables.  ey_tune_set returns EY_EINVAL for an unknown name; ey_tune_get returns -1.
 * Process-wide, not synchronised: set them before the first launch. */
int ey_tune_set(const char* name, long value);
long ey_tune_get(const char* name);

/* ---- K1: dense convolution (+ folded-BN bias, activation, residual) as NHWC implicit GEMM on MFMA ------------
 * Replaces Conv.forward_fuse (nn/modules/conv.py:57-59, BN folded by utils/torch_utils.py:238-265), the raw
 * nn.Conv2d+bias calls of the heads (nn/modules/head.py:61,70) and LinearAttention.qkv/proj (block.py:3357-3358);
 * also absorbs nn.Upsample(nearest x2)+Concat feeding a conv (yaml layers 11-12,14-15,18,21; conv.py:353-355),
 * Bottleneck/PSA residual adds (block.py:480,3446-3449) and the _WaveletEnhancer tail (block.py:3706-3710).
 *
 *   y = res + out_scale * act( conv_k(cat_c(src0, src1)) + bias + bilinear_up2x(addz) )
 *
 * src[i] may be read through a nearest x2^up upsample (src_up = 0|1).  k in {1,3}, stride in {1,2}, pad = k/2.
 * `ngroup` > 1 runs over `ngroup` channel-offset slices (src0 += g*src_gstride, y += g*y_gstride elements) with
 * weight set min(g, w_gmax) — the three high-frequency sub-bands share f_h, and f_ll (a 1x1 conv written as a
 * centre-tap 3x3) rides in the same launch as group 0 (block.py:3688-3694).
 * Weights must be packed by ey_conv_pack_weight(). */
typedef struct {
  int32_t dtype;
  int32_t B, H, W;   /* logical conv input extent (after the virtual upsample) */
  int32_t Ho, Wo;    /* output extent */
  int32_t Cout;
  int32_t k, stride, pad;
  int32_t act;
  int32_t nsrc;      /* 1 or 2 */
  const void* src[2];
  int32_t src_C[2];
  int32_t src_cstride[2];
  int32_t src_up[2];
  const void* w;     /* packed, see ey_conv_pack_weight */
  const float* bias; /* [Cout] fp32 or NULL */
  void* y;
  int32_t y_cstride;
  const void* res;   /* optional, [B,Ho,Wo,Cout] view, same dtype */
  int32_t res_cstride;
  float out_scale;   /* 1.0f unless the wavelet tail (tanh(gamma)) */
  const void* addz;  /* optional, [B,addz_H,addz_W,Cout] view, bilinearly resized (align_corners=False) to Ho x Wo */
  int32_t addz_cstride;
  int32_t addz_H, addz_W;
  int32_t ngroup;
  int64_t src_gstride, y_gstride;
  /* group g uses weight set min(g, w_gmax): w + that*w_gstride (elements of dtype), bias + that*Cout.  0/0 = shared. */
  int64_t w_gstride;
  int32_t w_gmax;
} ey_conv_desc;

/* Bytes of the packed weight buffer for a conv with Cout x (k*k*Cin) (Cin = sum of src_C). */
size_t ey_conv_packed_bytes(int dtype, int Cout, int Cin, int k);
/* host -> host: w_oihw fp32 [Cout][Cin][k][k]  ->  packed rows [Cout_pad][k][k][Cin] (+ row permutation for the
 * MFMA epilogue, + zero slack).  Upload `out` to the device afterwards. */
int ey_conv_pack_weight(int dtype, int Cout, int Cin, int k, const float* w_oihw_host, void* out_host, size_t out_bytes);
int ey_conv2d(const ey_conv_desc* d, ey_stream_t stream);
/* Kernel instantiation ey_conv2d launches for a shape (profiling only): kind*1000 + NT*10 + MT, kind 3 =
 * conv_small_kernel<T,NT,BATCH> (small-M latency kernel), 2 = conv3_halo_kernel<T,NT,stride> (3x3, LDS halo tile),
 * 1 = conv_ws_kernel<T,NT,MT,k> (weight-stationary persistent), 0 = conv_igemm_kernel<T,NT,MT> (K-chunked fallback).
 * plain_single_source = one source, no upsample.  A prediction for tools: it ignores the tunables and the kernels tried
 * before these; ey_conv_last_variant() reports what a launch actually ran. */
int ey_conv_variant(int dtype, int Cout, int Cin, int k, int stride, int plain_single_source, long M, int ngroup);
/* Code of the kernel the last ey_conv2d on this thread launched (every launch path reports it; 0 before any launch):
 * 3000 + KS*10 + NTW = conv_pwn_kernel<KS,NTW>; 4000 + NT*10 + nsrc = conv_pw_kernel<T,NT,...>; 5000 + NT*10 + KS =
 * conv_pwr_kernel<T,NT,KS,...>; 6000 + NT*10 + stride = conv3_tile_kernel<T,NT,S,...>; 7000 + NT*10 + stride = conv3r_kernel<NT,S>;
 * 8000 + NT*100 + MT*10 + stride = conv3s_kernel<NT,MT,...>; 9000 + NT*10 + fast = conv3p_kernel<NT,FAST>;
 * 10000 + NT*10 + BATCH = conv_small_kernel<T,NT,BATCH>; 11000 + NT*10 + stride = conv3_halo_kernel<T,NT,S>;
 * 12000 + NT*100 + MT*10 + k = conv_ws_kernel<T,NT,MT,k>; 13000 + NT*10 + MT = conv_igemm_kernel<T,NT,MT>.  Profiling labels / tests. */
int ey_conv_last_variant(void);
/* ---- two chained pointwise convs in one kernel, registers only: y = act2(W2 . act1(W1 . x + b1) + b2) -- the last two 1x1 convs
 * of the Detect class tower (Conv(c3,c3,1)+SiLU, nn.Conv2d(c3,nc,1); head.py:68-70).  w1_packed = ey_conv_pack_weight(Cmid, Cin, 1);
 * w2_packed = ey_conv_pack_weight(Cout, ey_conv_chain_klen(Cmid), 1) of W2 with its INPUT columns gathered by ey_conv_chain_kperm
 * (perm[k'] = mid channel feeding k-slot k', -1 = zero column): the second contraction runs in the order the first GEMM leaves its
 * results in the registers.  f16 only; built for the two class-tower shapes Cin 72..96 -> Cmid 80 -> Cout <= 80 (nc = 80) and Cin 40..64 ->
 * Cmid 64 -> Cout <= 16 (small class counts, e.g. GC10-DET nc = 10); EY_EUNSUPPORTED otherwise (run the two convs). */
int ey_conv_chain_klen(int Cmid);
int ey_conv_chain_kperm(int Cmid, int* perm_host, int perm_len);
int ey_conv_pw_chain(int dtype, int B, int H, int W, int Cin, int Cmid, int Cout, const void* x, int x_cstride, const void* w1_packed,
                     const float* b1, int act1, const void* w2_packed, const float* b2, int act2, void* y, int y_cstride, ey_stream_t stream);
/* NT the weights of a Cout-channel conv are packed with (row permutation of ey_conv_pack_weight). */
int ey_conv_pack_nt(int Cout);

/* ---- generic direct convolution (any Cin/Cout/groups/k/stride; scalar) — correctness path for shapes the MFMA
 * kernel does not take (channel counts not multiples of 8, grouped convs).  Weights: fp32 OIHW on device. */
typedef struct {
  int32_t dtype;
  int32_t B, H, W, Cin, Ho, Wo, Cout;
  int32_t k, stride, pad, groups, act;
  const void* x; int32_t x_cstride;
  const float* w_oihw; const float* bias;
  void* y; int32_t y_cstride;
} ey_conv_direct_desc;
int ey_conv2d_direct(const ey_conv_direct_desc* d, ey_stream_t stream);

/* ---- stem: 3x3 stride-2 conv on the NCHW input image -> NHWC, + bias + SiLU (layer 0; conv.py:41-59).
 * x: [B,Cin,H,W] contiguous, x_dtype EY_F16|EY_F32; w: fp32 [Cout][Cin][3][3] device; Cin<=4, Cout%16==0. */
int ey_stem_conv(int x_dtype, int y_dtype, int B, int Cin, int H, int W, int Cout, int act, const void* x_nchw,
                 const float* w_oihw, const float* bias, void* y, int y_cstride, ey_stream_t stream);
/* The same contract for the other image stems: (k, stride, pad) = (6, 2, 2) (YOLOv5's Conv(3, c, 6, 2, 2)), (3, 1, 1) (YOLOv3's
 * Conv(3, c, 3, 1)) and (7, 2, 3) (the ResNet stem, K = 147 zero-filled to 160 on the MFMA); w: fp32 [Cout][Cin][k][k] device.  Ho = (H + 2 pad - k) / stride + 1: the 6x6 window of output o covers the input
 * columns 2o - 2 ... 2o + 3.  f16 -> f16 with Cin = 3, W % 8 == 0, a 16-byte aligned image and Cout <= 80 runs on the MFMA (weights rounded to
 * f16); everything else on the exact fp32 VALU form.  EY_EUNSUPPORTED (before anything is launched) for every other (k, stride, pad).
 * ey_stem_conv_ks_last_variant: 1 when the last launch took the MFMA form, 0 for the VALU form (developer tools, tests). */
int ey_stem_conv_ks(int x_dtype, int y_dtype, int B, int Cin, int H, int W, int Cout, int k, int stride, int pad, int act, const void* x_nchw,
                    const float* w_oihw, const float* bias, void* y, int y_cstride, ey_stream_t stream);
int ey_stem_conv_ks_last_variant(void);

/* ---- nn.MaxPool2d(k, stride) behind an explicit nn.ZeroPad2d((pad_l, pad_r, pad_t, pad_b)) (yolov3-tiny): the padded cells take part in the
 * maximum with value 0 -- not -inf -- so an all-negative border gives 0.  k = 2 with stride 1 or 2; k = 1, stride 1 is the zero-padded copy
 * (a lone ZeroPad2d).  Ho = (H + pad_t + pad_b - k) / stride + 1 (floor: an odd last row / column is dropped at stride 2).  x and y are
 * 16-byte aligned channel windows of NHWC buffers, C a multiple of 8.  Bit-identical to torch's max_pool2d of the padded map for finite
 * inputs.  EY_EUNSUPPORTED for every other (k, stride). */
int ey_maxpool2d(int dtype, int B, int H, int W, int C, int k, int stride, int pad_l, int pad_r, int pad_t, int pad_b, const void* x, int x_cstride,
                 void* y, int y_cstride, ey_stream_t stream);

/* ---- nn.MaxPool2d(3, 2, 1) of the ResNet stem (csrc/resnet.hip): torch's own padding, i.e. the cells outside the map are LEFT OUT of the
 * maximum (ey_maxpool2d's zero ring takes part in it).  Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1.  x [B,H,W,*] and y [B,Ho,Wo,*] are 16-byte
 * aligned channel windows of NHWC buffers of `dtype` (EY_F16 | EY_F32), C a multiple of 8: EY_EUNSUPPORTED before any launch otherwise.  The
 * window is walked row by row and a cell replaces the running maximum only when it is greater, as torch's CPU kernel does: bit-identical to
 * F.max_pool2d(x, 3, 2, 1). */
int ey_maxpool3x3s2(int dtype, int B, int H, int W, int C, const void* x, int x_cstride, void* y, int y_cstride, ey_stream_t stream);
/* Layer 0 of a ResNet as ONE launch (csrc/resnet.hip): Conv 7x7 / 2 / 3 + bias + activation from the planar NCHW image into an LDS tile of the
 * half-resolution 64-channel map, nn.MaxPool2d(3, 2, 1) from that tile; only the quarter-resolution map y [B,Hp,Wp,*] is written,
 * Hp = ((H - 1) / 2) / 2 + 1.  The convolution runs on the device functions of ey_stem_conv_ks: bit-identical to ey_stem_conv_ks(7, 2, 3)
 * followed by ey_maxpool3x3s2, in the MFMA form (f16, Cin = 3, W % 8 == 0, 16-byte aligned image) and the VALU form (fp32, or f16 otherwise).
 * x_dtype == y_dtype, Cin 1..4, Cout = 64, y a 16-byte aligned channel slot; w fp32 [64][Cin][7][7], bias fp32: EY_EUNSUPPORTED before any
 * launch otherwise.  Up to 128 KiB of dynamic LDS.  ey_resnet_stem_last_variant: 1 = MFMA form, 0 = VALU form (developer tools, tests). */
int ey_resnet_stem(int x_dtype, int y_dtype, int B, int Cin, int H, int W, int Cout, int act, const void* x_nchw, const float* w_oihw, const float* bias, void* y,
                   int y_cstride, ey_stream_t stream);
int ey_resnet_stem_last_variant(void);
/* The closing 1x1 of a ResNet bottleneck block (csrc/resnet.hip), f16 on the MFMA: y = relu(W [t ; x|s] + b + res), the residual added in fp32
 * BEFORE the activation, one f16 rounding.  t: [B,Ho,Wo,*] with C2 channels (C2 = 64 | 128 | 256 | 512), y: [B,Ho,Wo,*] with 4 C2 channels,
 * Ho = (H - 1) / stride + 1.  Identity block: C1 = 0, x NULL, stride 1, w DEVICE f16 [4 C2][C2] row-major, res [B,Ho,Wo,*] = the block input.
 * Projection block: x [B,H,W,*] with C1 channels (a multiple of 32 up to 2048) is read at pixel (stride oy, stride ox), stride 1 | 2, w is
 * [W3 | Ws] concatenated along K ([4 C2][C2 + C1]), bias = b3 + bs (fp32, 16-byte aligned), res NULL: the shortcut conv's output never exists.
 * Sources 16-byte, y and res 8-byte aligned channel slots.  EY_EUNSUPPORTED before any launch for fp32 and every other shape. */
int ey_resnet_tail(int dtype, int B, int H, int W, int stride, int C1, int C2, const void* t, int t_cstride, const void* x, int x_cstride, const void* w,
                   const float* bias, const void* res, int res_cstride, void* y, int y_cstride, ey_stream_t stream);

/* ---- two chained 1x1 convs as one launch (f16, 64 or 128 channels, small maps): `second` must read exactly what `first` writes
 * (second->src[0] == first->y, same cstride, one source each; `first` may carry bias / addz / activation / out_scale / residual, `second`
 * bias / activation).  Built for the _WaveletEnhancer tail conv (block.py:3700-3710) + the stacked cv1|cv2 conv of the DSC3k behind it
 * (block.py:382-396).  Both outputs are written; bit-identical to two ey_conv2d calls.  EY_EUNSUPPORTED (nothing launched) otherwise. */
int ey_conv_pw_pair(const ey_conv_desc* first, const ey_conv_desc* second, ey_stream_t stream);

/* ---- a block's closing 1x1 conv over a two-part virtual concat + the stride-2 3x3 conv behind it, as one kernel (f16; Cmid = Cout = 64;
 * C0, C1 <= 32, multiples of 8; both bias + SiLU):   y = act2( Conv3x3s2( act1( Conv1x1( cat(src0, src1) ) + bias1 ) ) + bias2 )
 * = DSC3K2_Wavelet.cv2 / C2f.cv2 (block.py:357-396,3783-3788) + the next backbone layer Conv(64,64,3,2) (conv.py:41-59).  The (B,64,H,W)
 * map between them stays in LDS, rounded to f16 as ey_conv2d stores it: bit-identical to the two ey_conv2d calls.  w1: ey_conv_pack_weight
 * (EY_F16, 64, C0 + C1, 1), w2: (EY_F16, 64, 64, 3).  EY_EUNSUPPORTED (before anything is launched) for every other shape. */
int ey_conv_pw_conv3s2(int dtype, int B, int H, int W, const void* src0, int C0, int cstride0, const void* src1, int C1, int cstride1, int Cmid,
                       const void* w1_packed, const float* bias1, int act1, int Cout, const void* w2_packed, const float* bias2, int act2, void* y,
                       int y_cstride, ey_stream_t stream);

/* ---- layers 0 + 1 as one kernel (f16): y = act1( Conv3x3s2_{16->C1}( act0( Conv3x3s2_{3->16}(x) + bias0 ) ) + bias1 ), conv.py:41-59 twice.
 * x: [B,3,H,W] contiguous f16 (W % 8 == 0); w0: fp32 [16][3][3][3] device; w1: ey_conv_pack_weight(EY_F16, C1, 16, 3, ...); C1 = 32.
 * The (B,16,H/2,W/2) intermediate stays in LDS (rounded to f16 as ey_stem_conv stores it): bit-identical to ey_stem_conv + ey_conv2d.
 * EY_EUNSUPPORTED (before anything is launched) for every other shape. */
int ey_stem_pair(int B, int H, int W, const void* x_nchw, const float* w0_oihw, const float* bias0, int act0, int C1, const void* w1_packed,
                 const float* bias1, int act1, void* y, int y_cstride, ey_stream_t stream);

/* ---- K2/K3: depthwise kxk, stride 1, pad k/2 (+ optional bias + activation).  DSConv.dw (conv.py:94-97,102) and
 * DWConv (conv.py:124-129) in Detect.cv3 (head.py:68-69).  w: [k][k][C] in `dtype`; k in {3,5,7}; C%8==0. */
int ey_dwconv(int dtype, int B, int H, int W, int C, int k, int act, const void* x, int x_cstride, const void* w_kkc,
              const float* bias, void* y, int y_cstride, ey_stream_t stream);

/* ---- K2/K3 fused: depthwise kxk -> pointwise 1x1 in one kernel:
 *   y = res + act( pw1x1( dw_act( dw_kxk(x) + dw_bias ) ) + bias )
 * = DSConv.forward (conv.py:101-104; dw_bias NULL, dw_act NONE, BN folded into pw) and the Detect.cv3 pairs
 * DWConv(BN+SiLU) -> Conv 1x1 (head.py:68-69).  The depthwise result stays in LDS (rounded to `dtype` like the
 * reference's intermediate tensor).  w_dw: [k][k][Cin] in `dtype`; dw_bias fp32 [Cin] or NULL;
 * w_pw: ey_conv_pack_weight(dtype, Cout, Cin, 1, ...); k in {3,5,7}; Cin%8==0, Cin<=256. */
int ey_dsconv(int dtype, int B, int H, int W, int Cin, int Cout, int k, int act, const void* x, int x_cstride,
              const void* w_dw_kkc, const float* dw_bias, int dw_act, const void* w_pw_packed, const float* bias, void* y, int y_cstride, const void* res,
              int res_cstride, ey_stream_t stream);

/* Toeplitz form of the depthwise stage for wide kernels (k = 7; f16; Cin 16 or 32, Cout <= 32): the row filter becomes one
 * 16x16x32 MFMA per channel and filter row (7 MFMAs per channel per 16x16 tile instead of 12544 FMAs).  w_dw_toeplitz is
 * built once on the host by ey_dsconv_pack_toeplitz from the fp32 [k][k][C] depthwise weights (ey_dsconv_toeplitz_bytes bytes,
 * then uploaded).  Same arguments and result as ey_dsconv; shapes outside the Toeplitz kernel are forwarded to ey_dsconv. */
size_t ey_dsconv_toeplitz_bytes(int C, int k);
int ey_dsconv_pack_toeplitz(int C, int k, const float* w_dw_kkc_host, void* out_host, size_t out_bytes);
int ey_dsconv_tz(int dtype, int B, int H, int W, int Cin, int Cout, int k, int act, const void* x, int x_cstride,
                 const void* w_dw_kkc, const void* w_dw_toeplitz, const float* dw_bias, int dw_act, const void* w_pw_packed, const float* bias,
                 void* y, int y_cstride, const void* res, int res_cstride, ey_stream_t stream);

/* ---- K2 pair: DSBottleneck.forward (block.py:1496-1503) as one kernel on small maps (f16; C = c1 = c_ = c2 in {32, 64}; k1 = 3,
 * k2 in {5, 7}; stride 1):   y = [x +] DSConv_k2( DSConv_k1(x) ),  DSConv_k(t) = act( pw1x1( dw_kxk(t) ) + bias ).
 * A workgroup owns a band of rows of one image and recomputes the first DSConv on the second one's halo rows; the intermediate
 * tensor stays in LDS, rounded to f16 exactly as the two-launch form (2 x ey_dsconv) stores it: the result is bit-identical to that
 * form.  Weights as for ey_dsconv (no depthwise bias).  Returns EY_EUNSUPPORTED -- before anything is launched -- for every other
 * shape; the caller then issues the two ey_dsconv calls. */
int ey_dsb_pair(int dtype, int B, int H, int W, int C, int k1, int k2, int act, const void* x, int x_cstride, const void* w_dw1_kkc,
                const void* w_pw1_packed, const float* bias1, const void* w_dw2_kkc, const void* w_pw2_packed, const float* bias2, int add_residual,
                void* y, int y_cstride, ey_stream_t stream);

/* Kernel the last ey_dsconv / ey_dsconv_tz on this thread launched (profiling labels): 1 = dsconv_kernel (LDS tile),
 * 2 = dsconv_strip_kernel (register strip), 3 = dsconv_tz_kernel (Toeplitz MFMA). */
int ey_dsconv_last_variant(void);

/* ---- K4: single-level 2-D Haar analysis (_PywtDWT2D.forward, block.py:3619-3642).
 * x [B,H,W,C] -> y [B,H/2,W/2,4C] with channel blocks LL|LH|HL|HH; odd H/W floor like the stride-2 conv. */
int ey_dwt_haar(int dtype, int B, int H, int W, int C, const void* x, int x_cstride, void* y, int y_cstride,
                ey_stream_t stream);

/* ---- K4 (any filter bank): single-level 2-D analysis with a k-tap pywt bank (_PywtDWT2D, block.py:3582-3642):
 * F.pad(mode="reflect", pad = k/2 - 1), then a depthwise k x k conv with stride 2 and no padding.  The padded map is never built
 * (reflect indexing).  x [B,H,W,C] -> y [B,H/2,W/2,4C] with channel blocks LL|LH|HL|HH, as ey_dwt_haar.  taps: DEVICE fp32
 * [4][k][k] = (LL, LH, HL, HH) outer products of h0 = dec_lo[::-1] and h1 = dec_hi[::-1] (LH: rows h0, columns h1), each rounded
 * once in fp32 and then to the activation dtype, as the reference convolves with.  k even, 2..64.  EY_EINVAL (nothing launched)
 * when pad >= H or pad >= W: torch refuses that reflect padding too. */
int ey_dwt(int dtype, int B, int H, int W, int C, int k, const float* taps, const void* x, int x_cstride, void* y, int y_cstride,
           ey_stream_t stream);

/* ---- K4+K5 fused: the half-resolution branch of _WaveletEnhancer (block.py:3688-3706) in one kernel (f16 only):
 *   Z = W_z . cat[ SiLU(f_ll(LL)+b), SiLU(f_h(LH)+b), SiLU(f_h(HL)+b), SiLU(f_h(HH)+b) ]   with (LL,LH,HL,HH) = Haar DWT of x
 * x [B,H,W,C] -> z [B,H/2,W/2,C].  w_sub_packed: two ey_conv_pack_weight(EY_F16, C/2, C, 3) sets w_set_stride ELEMENTS apart (set 0 =
 * f_ll written as a centre-tap 3x3, set 1 = the shared f_h); b_sub fp32 [2][C/2]; w_z_packed = ey_conv_pack_weight(EY_F16, C, 2C, 1)
 * (the fuse conv's columns over the processed sub-bands with the band weights folded in).  C in {16,32,64,128}; EY_EUNSUPPORTED
 * otherwise / for fp32 (run ey_dwt_haar + ey_conv2d x2).  Replaces three launches and the HBM round trip of the 4C-channel sub-band
 * tensor and the 2C-channel P. */
int ey_wavelet_z(int dtype, int B, int H, int W, int C, const void* x, int x_cstride, const void* w_sub_packed, long w_set_stride, const float* b_sub,
                 const void* w_z_packed, void* z, int z_cstride, ey_stream_t stream);
/* The same branch for a k-tap pywt bank and / or a DSConv f_h (_PywtDWT2D block.py:3582-3642 with reflect padding k/2 - 1;
 * _WaveletEnhancer(use_ds=True) block.py:3686).  ey_wavelet_z is this call with k = 2, taps = NULL, use_ds = 0.
 * k in {2, 4, 6, 8}; taps: DEVICE fp32 [4][k][k] as for ey_dwt (unused for k = 2, which is the Haar kernel).  use_ds: set 1 of
 * w_sub_packed is f_h's pointwise 1x1 (BN folded) written as a centre-tap 3x3, like f_ll, and w_dw_kkc the depthwise 3x3 weights,
 * DEVICE f16 [3][3][C], 16-byte aligned; the depthwise output is rounded to f16 like ey_dsconv's.  EY_EUNSUPPORTED (nothing launched)
 * for fp32, other C or other k; EY_EINVAL when k/2 - 1 >= H or >= W. */
int ey_wavelet_z2(int dtype, int B, int H, int W, int C, int k, const float* taps, int use_ds, const void* w_dw_kkc, const void* x, int x_cstride,
                  const void* w_sub_packed, long w_set_stride, const float* b_sub, const void* w_z_packed, void* z, int z_cstride, ey_stream_t stream);

/* ---- K6: the three chained 5x5/s1/p2 max-pools of SPPF (block.py:219-223): y1=mp(x), y2=mp(y1), y3=mp(y2). */
int ey_sppf_pool(int dtype, int B, int H, int W, int C, const void* x, int x_cstride, void* y1, void* y2, void* y3,
                 int y_cstride, ey_stream_t stream);

/* Per-channel layer scale with residual (A2C2f, reference block.py:1459-1463):  y[p][c] = x[p][c] + gamma[c] * t[p][c], the product
 * rounded to the activation dtype before the add as the reference does.  gamma: DEVICE fp32 [C].  y may alias t or x. */
int ey_scale_add_channels(int dtype, int B, int H, int W, int C, const void* x, int x_cstride, const float* gamma, const void* t, int t_cstride,
                          void* y, int y_cstride, ey_stream_t stream);

/* ---- SCDown of YOLOv10 (reference block.py:1174-1206) as one kernel (f16, k = 3):
 *     y = act2( DWConv_{3x3, s2, pad 1}( round_f16( act1( Conv1x1_{C1->C2}(x) + bias1 ) ) ) + bias2 ),   Ho = (H-1)/2 + 1
 * x and y are channel windows of NHWC buffers (x may be a slice, y a slot of a concat buffer).  w1: ey_conv_pack_weight(EY_F16, C2, C1, 1);
 * w2: [3][3][C2] f16 as ey_dwconv_s2 takes it; biases fp32, bias2 may be NULL.  The (B,C2,H,W) map between the two convs stays in LDS, rounded
 * to f16 as ey_conv2d stores it; taps outside the map are skipped as ey_dwconv_s2 skips them: bit-identical to ey_conv2d + ey_dwconv_s2.
 * Takes C1 % 8 == 0, C2 % 64 == 0, act1 none / ReLU / SiLU, act2 none / ReLU, 16-byte aligned views, any H, W >= 1; no workspace, no atomics.
 * EY_EUNSUPPORTED (before anything is launched) for everything else: the caller runs the two launches. */
int ey_scdown(int dtype, int B, int H, int W, int C1, int C2, int k, const void* x, int x_cstride, const void* w1_packed, const float* bias1, int act1,
              const void* w2_kkc, const float* bias2, int act2, void* y, int y_cstride, ey_stream_t stream);

/* ---- GhostConv(c1, 2 Ch, 1, 1) of the YOLOv8-ghost models (reference conv.py:180-193) as one kernel (f16, k = 5):
 *     y1 = round_f16( act( Conv1x1_{C1->Ch}(x) + bias1 ) ),   y2 = round_f16( act( DWConv_{5x5, s1, pad 2}(y1) + bias2 ) )
 *     y[:, 0:Ch] = y1, y[:, Ch:2Ch] = y2;   with res:  y = round_f16( f32(cat(y1, y2)) + f32(res) )   (an f16 add; y may be res itself)
 * x, y and res are channel windows of NHWC buffers (slices or slots of a concat buffer, each with its own pixel stride).
 * w1: ey_conv_pack_weight(EY_F16, Ch, C1, 1); w2: [5][5][Ch] f16 as ey_dwconv takes it; biases fp32, bias2 may be NULL; act (both convs) none,
 * ReLU or SiLU.  y1 stays in LDS, rounded to f16 as ey_conv2d stores it; the depthwise stage is ey_dwconv's arithmetic (sum started from the
 * bias, taps in (ky, kx) order, taps outside the map skipped): where Ch % 8 == 0 the result is bit-identical to ey_conv2d + ey_dwconv (+ the
 * f16 add).  Takes C1 % 8 == 0 (C1 <= 832), Ch % 4 == 0, any H, W >= 1; x 16-byte aligned, y and res 16-byte aligned, 8-byte where
 * Ch % 8 == 4; no workspace, no atomics.  EY_EUNSUPPORTED (before anything is launched) for everything else, f32 and k != 5 included: the
 * caller composes. */
int ey_ghost_conv(int dtype, int B, int H, int W, int C1, int Ch, int k, const void* x, int x_cstride, const void* w1_packed, const float* bias1,
                  const void* w2_kkc, const float* bias2, int act, const void* res, int res_cstride, void* y, int y_cstride, ey_stream_t stream);

/* ---- YOLOv13 (HyperACE / FullPAD, reference block.py:1564-2008, conv.py:87-104) --------------------------------------------------------
 * AvgPool2d(2) (FuseModule.downsample / DownsampleConv.downsample, block.py:1858,1985): y[b,i,j,c] = mean of the 2x2 window at (2i, 2j),
 * floor semantics (Ho = H/2, Wo = W/2; an odd last row / column is dropped), summed in fp32 in row-major order and rounded once.  x and y
 * are channel windows of NHWC buffers (y may be a slot of a concat buffer).  H, W >= 2. */
int ey_avgpool2(int dtype, int B, int H, int W, int C, const void* x, int x_cstride, void* y, int y_cstride, ey_stream_t stream);

/* Depthwise kxk, STRIDE 2, pad k/2 (DSConv(c1, c2, k, s=2).dw, conv.py:94-97; yolov13 layers 5 and 7): Ho = (H-1)/2 + 1.  w: [k][k][C]
 * in `dtype`; k in {3,5,7}; bias fp32 [C] or NULL; any C.  The 1x1 behind it runs on ey_conv2d.  Stride-1 depthwise is ey_dwconv. */
int ey_dwconv_s2(int dtype, int B, int H, int W, int C, int k, int act, const void* x, int x_cstride, const void* w_kkc, const float* bias,
                 void* y, int y_cstride, ey_stream_t stream);

/* Adaptive hypergraph convolution (AdaHGConv.forward, block.py:1765-1774, with AdaHyperedgeGen.forward, block.py:1686-1716) on the
 * N = H*W tokens of each of B images, x / y [B,N,D] channel windows (no transpose: a token is a pixel).  E hyperedges, `heads` heads
 * (head_dim = D/heads), context 0 "both" / 1 "mean" / 2 "max".  Y = GELU(node_proj(A . GELU(edge_proj(A^T X)))) + X with A = the softmax
 * over all N tokens of each hyperedge's logits.  Device weights, all fp32 except node_w:
 *   proto_base [E][D]; ctx_wT = context_net.weight^T [K][E*D] (K = 2D for "both", else D); ctx_b [E*D];
 *   pre_w = pre_head_proj.weight [D][D] (as stored: [out][in]); pre_b [D];  edge_wT = edge_proj[0].weight^T [D in][D out]; edge_b [D];
 *   node_w: f16 -> node_proj[0].weight in f16, [D out][Kp] with Kp = D rounded up to 32 and a zero tail (16-byte aligned); fp32 ->
 *   node_proj[0].weight^T [D in][D out];  node_b [D].
 * pre_head_proj is folded per image (logits = (X . P Wp^T' + P . bp) / (sqrt(head_dim) * heads)), so it costs N*D*E, not N*D*D.
 * Five launches; every reduction has a fixed order: bit-identical run to run.  f16: node_proj on MFMA with fp32
 * accumulation, softmax statistics and all intermediates in fp32, A.He' rounded to f16 as its operand.  fp32: exact fp32 VALU.
 * workspace: ey_hypergraph_workspace_bytes(B, N, D, E) bytes, 16-byte aligned; nothing is allocated and the host never waits, so the
 * call can be captured into a graph.  EY_EINVAL (nothing launched): D not a multiple of 16 in [16, 384], E not in [1, 16], heads not
 * dividing D, overlapping x / y windows, a short or misaligned workspace. */
size_t ey_hypergraph_workspace_bytes(int B, int N, int D, int E);
int ey_hypergraph_conv(int dtype, int B, int N, int D, int E, int heads, int context, const void* x, int x_cstride, void* y, int y_cstride,
                       const float* proto_base, const float* ctx_wT, const float* ctx_b, const float* pre_w, const float* pre_b,
                       const float* edge_wT, const float* edge_b, const void* node_w, const float* node_b, void* workspace,
                       size_t workspace_bytes, ey_stream_t stream);

/* ---- LGL block (LGLBlock = LocalAgg + SelfAttn, reference block.py:3042-3210; YOLOv13 DSC3K2_LGL, block.py:3213-3345) ------------------
 * All sums, gates and statistics below are fp32 in both storage types; x / y are channel windows of NHWC buffers.
 *
 * Depthwise kxk, stride 1, pad k/2, + bias with an epilogue (k in {3, 9}; C % 8 == 0; w: [k][k][C] in `dtype`, 32-byte aligned; bias fp32
 * [C] or NULL):  mode 0: y = dw(x) + b (LocalAgg.attn, block.py:3085,3094);  1: y = x + x * (sigmoid(dw(x) + b) - 1/2) (LocalAgg.pos_embed
 * and its gate, block.py:3081,3093);  2: y = x + dw(x) + b (SelfAttn.pos_embed, block.py:3180,3190).  ey_dwconv (k 3/5/7, no epilogue) is
 * unchanged. */
enum { EY_DWG_PLAIN = 0, EY_DWG_GATE = 1, EY_DWG_RESIDUAL = 2 };
int ey_dwconv_gate(int dtype, int B, int H, int W, int C, int k, int mode, const void* x, int x_cstride, const void* w_kkc, const float* bias,
                   void* y, int y_cstride, ey_stream_t stream);
/* y = x + x * (sigmoid(g) - 1/2): the gate of LocalAgg's second step, whose g is a 1x1 conv output (block.py:3094).  Any C; y may alias g. */
int ey_sigmoid_gate(int dtype, int B, int H, int W, int C, const void* x, int x_cstride, const void* g, int g_cstride, void* y, int y_cstride,
                    ey_stream_t stream);
/* Exact GELU, 0.5 x (1 + erf(x / sqrt 2)) (nn.GELU() behind Mlp.fc1, block.py:3047-3054).  Any C; y may alias x. */
int ey_gelu(int dtype, int B, int H, int W, int C, const void* x, int x_cstride, void* y, int y_cstride, ey_stream_t stream);
/* CMlp behind BatchNorm, per channel (LocalAgg step 3, block.py:3060-3076,3095): a = scale[c] * x + shift[c] inside the map and ZERO outside
 * (the reference zero-pads the BatchNorm output, so the affine cannot be folded into the weights); hidden_j = GELU(b1[j][c] + 3x3(a; w1[j]))
 * for the r hidden maps of channel c (fc1 = Conv2d(C, rC, 3, pad 1, groups=C): output channel c*r + j), zero outside the map (fc2's padding);
 * o = b2[c] + sum_j 3x3(hidden_j; w2[j]) (fc2 = Conv2d(rC, C, 3, pad 1, groups=C)).  The hidden maps stay in registers.  gate != 0:
 * y = x + x * (sigmoid(o) - 1/2), else y = o.  Device fp32: scale / shift [C] or NULL (identity), w1 / w2 [r][9][C], b1 [r][C], b2 [C];
 * r in 1..8; any C. */
int ey_cmlp(int dtype, int B, int H, int W, int C, int r, int gate, const void* x, int x_cstride, const float* scale, const float* shift,
            const float* w1, const float* b1, const float* w2, const float* b2, void* y, int y_cstride, ey_stream_t stream);
/* nn.LayerNorm(C) over the channels of each pixel (SelfAttn.norm1 / norm2, block.py:3181,3185,3193-3194): two-pass fp32 mean and variance
 * on registers, y = (x - mean) / sqrt(var + eps) * gamma + beta; C a multiple of 8 up to 384; gamma, beta fp32 [C].  pool != 0: followed by
 * AvgPool2d(2, 2, ceil_mode=True) of the normalised values (GlobalSparseAttn.sampler, block.py:3120,3140) in the same kernel: y is
 * [B, ceil(H/2), ceil(W/2), C], a partial window divides by its in-bounds count.  ey_avgpool2 (floor mode) is unchanged. */
int ey_layernorm_channels(int dtype, int B, int H, int W, int C, float eps, int pool, const void* x, int x_cstride, const float* gamma,
                          const float* beta, void* y, int y_cstride, ey_stream_t stream);
/* GlobalSparseAttn.LocalProp + norm (block.py:3122-3123,3155-3162): depthwise ConvTranspose2d(k 2, s 2, no bias) of t [B,Hs,Ws,C]
 * (U[2i+a][2j+b][c] = t[i][j][c] * w[a][b][c]; w_abc fp32 [2][2][C]), a bilinear resize (align_corners=False) of U to H x W only when
 * (2Hs, 2Ws) != (H, W), then LayerNorm over channels: y [B,H,W,C].  Hs = ceil(H/2), Ws = ceil(W/2); C as ey_layernorm_channels. */
int ey_unpool2_layernorm(int dtype, int B, int Hs, int Ws, int H, int W, int C, float eps, const void* t, int t_cstride, const float* w_abc,
                         const float* gamma, const float* beta, void* y, int y_cstride, ey_stream_t stream);

/* ---- DySample (reference ultralytics/nn/modules/dysample.py), scale 2: offsets and bilinear gather in one kernel.
 *   O[n] = (w_offset[n] . x[b,h,w,:] + bias[n]) * 0.25 + init_pos[n]                          (w_scope == NULL)
 *   O[n] = (w_offset[n] . x[b,h,w,:] + bias[n]) * sigmoid(w_scope[n] . x[b,h,w,:]) * 0.5 + init_pos[n]
 * for the 8 * groups offset channels n = xy * 4 groups + grp * 4 + i * 2 + j (xy 0: x, 1: y), then for group grp's channels
 * [grp * C / groups, (grp + 1) * C / groups):   y[b, 2h+i, 2w+j, c] = bilinear sample of x[b, :, :, c] at column clamp(w + O_x, 0, W-1), row
 * clamp(h + O_y, 0, H-1), the upper neighbour index clamped to the map (F.grid_sample, align_corners=False, padding_mode="border").
 * w_offset / w_scope: DEVICE [8 groups][C] in `dtype`, 16-byte aligned (the 'pl' style is this form with a block-sparse weight);
 * bias / init_pos: DEVICE fp32 [8 groups].  The GEMM accumulates in fp32 (f16: MFMA; fp32: the exact f32 MFMA); offsets, coordinates
 * and the blend are fp32 in both storage types, the offset map stays in LDS.  x [B,H,W,*] and y [B,2H,2W,*] are channel windows of NHWC
 * buffers; only y's window is written.  Any H, W >= 1, any C with C / groups a multiple of 8.  EY_EUNSUPPORTED (before anything is
 * launched) for scale != 2, groups outside {2, 4, 8}, C / groups not a multiple of 8, x or y not 16-byte aligned windows. */
int ey_dysample(int dtype, int B, int H, int W, int C, int scale, int groups, const void* x, int x_cstride, const void* w_offset, const float* bias,
                const void* w_scope, const float* init_pos, void* y, int y_cstride, ey_stream_t stream);

/* ---- YOLO-World: max-sigmoid attention of C2fAttn (reference ultralytics/nn/modules/block.py:558-576, behind the `gl` linear and proj_conv).
 *   aw[b,m,p]     = sigmoid( max_n( sum_c e[b,p,m*hc+c] * g[bg,n,m*hc+c] ) / sqrt(hc) + bias[m] ) * scale[m]
 *   y[b,p,m*hc+c] = p[b,p,m*hc+c] * aw[b,m,p]
 * e, p, y: channel windows [B,HW,*] of NHWC buffers in `dtype` with their pixel strides, C = nh * hc channels used; only y's window is
 * written and nothing outside e's and p's windows is read.  g: DEVICE [Bg][n][C] in `dtype`, dense; Bg = 1 (one vocabulary for the batch,
 * bg = 0) or Bg = B (bg = b).  bias: DEVICE fp32 [nh]; scale: DEVICE fp32 [nh] or NULL (1.0).  The dot accumulates in fp32 (f16: one
 * mfma_f32_16x16x32_f16 per 16 pixels x 16 texts; fp32: an fmaf chain), the division is by the fp32 value of sqrt(hc), the tail is
 * fp32 and rounds once to storage.  1 <= n <= EY_MSA_MAX_TEXTS; text tiles past n repeat text n-1, so padding never enters the maximum.
 * No atomics and no workspace: deterministic and graph-capturable.  EY_EINVAL for a null pointer, n < 1 or a Bg other than 1 or B;
 * EY_EUNSUPPORTED (before anything is launched) for hc != 32, C != 32 * nh, n > EY_MSA_MAX_TEXTS, e / p / y / g not 16-byte aligned
 * windows, or a view of 2 GiB and more. */
#define EY_MSA_MAX_TEXTS 4096
int ey_max_sigmoid_attn(int dtype, int B, int HW, int nh, int hc, int C, int n, int Bg, const void* e, int e_cstride, const void* p, int p_cstride,
                        const void* g, const float* bias, const float* scale, void* y, int y_cstride, ey_stream_t stream);

/* ---- YOLOv9 (GELAN): the pooling front end of ADown / AConv (reference ultralytics/nn/modules/block.py:753-784) in one launch.
 *   A = avg_pool2d(x, 2, 1, 0)                 [B, H-1, W-1, C]; each window summed in fp32 as ((x00 + x01) + x10) + x11, times 0.25f, rounded
 *                                               once to `dtype` (bit-identical to torch's CPU avg_pool2d)
 *   a = A[..., :c_avg]                          [B, H-1, W-1, c_avg], the input of the 3x3 stride-2 conv
 *   m = max_pool2d(A[..., c_avg:], 3, 2, 1)     [B, H/2, W/2, C - c_avg], the maximum over the ROUNDED A values; window positions outside A are
 *                                               skipped.  These A values are never written to memory.
 * x, a, m: channel windows of NHWC buffers with their pixel strides.  c_avg == C is the AConv mode (m unused, may be NULL); c_avg == 0 is
 * refused.  H, W >= 2.  No atomics, no workspace: deterministic and graph-capturable.  EY_EINVAL unless C, c_avg and the strides are multiples
 * of 8 elements and the pointers 16-byte aligned; EY_EUNSUPPORTED when three rows of A of 8 channels exceed 64 KiB of LDS. */
int ey_adown_pool(int dtype, int B, int H, int W, int C, int c_avg, const void* x, int x_cstride, void* a, int a_cstride, void* m, int m_cstride,
                  ey_stream_t stream);

/* CBFuse (block.py:821-833): y[b,r,q,c] = sum_i src_i[b, ri(r), qi(q), c], every source resized to H x W with PyTorch's mode="nearest" rule
 *   ri(r) = min((int)floorf(r * ((float)Hi / (float)H)), Hi - 1),   qi(q) likewise from Wi and W   (any ratio; Hi == H reads at the identity).
 * The sum is fp32 in list order starting from source 0 and rounds once to `dtype`.  srcs: HOST array of n descriptors, 1 <= n <=
 * EY_CBFUSE_MAX, each a C-channel window [B, Hi, Wi, *] of an NHWC buffer with its pixel stride; they travel to the kernel by value.
 * EY_EINVAL unless C and all strides are multiples of 8 elements and all pointers 16-byte aligned. */
#define EY_CBFUSE_MAX 6
typedef struct ey_cbfuse_src {
  const void* ptr;
  int cstride, Hi, Wi;
} ey_cbfuse_src;
int ey_cbfuse(int dtype, int B, int H, int W, int C, int n, const ey_cbfuse_src* srcs, void* y, int y_cstride, ey_stream_t stream);

/* ---- Instance segmentation: mask assembly (utils/ops.py:644-693 process_mask + crop_mask, called by models/yolo/segment/predict.py:50-57).
 * For each of N kept detections (over the whole batch):
 *   v[r][c]   = sum_k coef_n[k] * proto[img_n, r, c, k]        fp32, k ascending, on the low-resolution grid mh x mw
 *   v[r][c]   = 0 unless  c >= x1/s, c < x2/s, r >= y1/s, r < y2/s   (crop_mask; the box scaled by 1/s in fp32)
 *   out[n]    = bilinear_{align_corners=False}(v -> s mh x s mw) > 0        as uint8 0 / 1   (s = 1: v > 0, no interpolation)
 * The interpolation reads source coordinate (dst + 0.5) / s - 0.5 clamped at 0, the upper neighbour clamped to the map (F.interpolate).
 * proto: NHWC [B, mh, mw, nm] window in `dtype`.  Coefficients: `nlevels` NHWC maps [B, H[l], W[l], nm] in `coef_dtype` as the cv4 towers of
 * Segment (nn/modules/head.py:358,365) write them; coef / coef_cstride / H / W are HOST arrays of length nlevels.  rows: DEVICE int32 [N][2] =
 * (image, anchor index in the concatenated order of the levels); boxes: DEVICE fp32 [N][4] x1,y1,x2,y2 in network-input pixels.
 * out: DEVICE uint8 [N][s mh][s mw]; every byte of it is written.  A row whose image or anchor is out of range gives an all-zero mask.
 * Low-resolution products stay in LDS.  EY_EUNSUPPORTED (nothing launched, nothing written) unless s in {1, 2, 4, 8}, nm a multiple of 8 up
 * to 64 and 1 <= nlevels <= 4.  N == 0 launches nothing. */
int ey_process_mask(int dtype, int B, int mh, int mw, int nm, const void* proto, int proto_cstride, int nlevels, const void* const* coef,
                    int coef_dtype, const int* coef_cstride, const int* H, const int* W, int N, const int* rows, const float* boxes, int s,
                    uint8_t* out, ey_stream_t stream);

/* ---- Instance segmentation at the original resolution (utils/ops.py:696-737 process_mask_native + scale_masks + crop_mask, behind
 * retina_masks=True in models/yolo/segment/predict.py:48-50 and process_mask_native in segment/val.py:52).  For each of N kept detections of a
 * batch of B images, image b with the record geo[b] = (top, bottom, left, right, H0, W0):
 *   v[r][c]    = sum_k coef_n[k] * proto[b, r, c, k]                          fp32, k ascending (as ey_process_mask)
 *   v          = v[top:bottom, left:right]                                    scale_masks' crop of the proto grid
 *   V[oy][ox]  = bilinear_{align_corners=False}(v -> H0 x W0)                 any ratio, up or down; per-axis index and weights of ey_scale_masks,
 *                fl(fl(l0y * fl(fl(l0x * a) + fl(l1x * b))) + fl(l1y * fl(fl(l0x * c) + fl(l1x * d))))
 *   out[oy][ox] = V > 0 and ox >= x1 and ox < x2 and oy >= y1 and oy < y2     crop_mask AFTER the resize, fp32 comparisons, as uint8 0 / 1
 * proto, coef, coef_dtype, coef_cstride, H, W, rows: as for ey_process_mask.  boxes: DEVICE fp32 [N][4] x1,y1,x2,y2 in ORIGINAL-image pixels
 * of the row's image (after scale_boxes, clipping included).  HOST arrays: mask_off (B + 1 entries, [0] == 0, non-decreasing, [B] == N): image
 * b owns rows mask_off[b] .. mask_off[b+1] - 1; geo [B][6] as _ops.mask_geometry / ey_mask_prompt state it (the images may all differ);
 * out_off [B]: image b's masks are the bytes out[out_off[b] .. out_off[b] + N_b H0 W0) viewed as (N_b, H0, W0), every one of them is written
 * and nothing else; all output indexing is 64-bit.  A row whose image is not the one that owns it, or whose anchor is out of range, gives
 * an all-zero mask and reads nothing; so does a box with a NaN corner.  N == 0 launches nothing.
 * One launch: a workgroup owns (detection, band of output rows), keeps the low-resolution pixels a tile blends in LDS as fp32, and stores 16
 * result bytes at a time wherever the address is a multiple of 16.  Tiles shrink with the ratio; where the original is smaller than half the crop
 * (or a tile's sources would not fit the LDS) the four products of a pixel are read from proto directly, so no ratio is refused.  No
 * atomics, fixed summation order: the same bytes run to run.
 * EY_EUNSUPPORTED (nothing launched, nothing written): nm not a multiple of 8 up to 64, nlevels outside 1..4, B > 64, a target side of 2^24 or more,
 * 2^31 or more work items.  EY_EINVAL: null pointers with N > 0, H0 or W0 < 1, an empty or misplaced crop (top >= bottom, left >= right: the
 * reference's F.interpolate fails there too), offsets that do not group the rows by image. */
int ey_process_mask_native(int dtype, int B, int mh, int mw, int nm, const void* proto, int proto_cstride, int nlevels, const void* const* coef,
                           int coef_dtype, const int* coef_cstride, const int* H, const int* W, int N, const int* rows, const float* boxes,
                           const int* mask_off, const int* geo, const long* out_off, uint8_t* out, ey_stream_t stream);

/* ---- Dense transposed convolution k 2, s 2 with bias: Proto.upsample = nn.ConvTranspose2d(c_, c_, 2, 2, 0, bias=True) (nn/modules/block.py:123,129).
 *   y[b, 2i+di, 2j+dj, co] = bias[co] + sum_ci x[b, i, j, ci] * W[ci][co][di][dj]
 * as one GEMM [B H W x Cin] . [Cin x 4 Cout] whose epilogue scatters the four positions.  f16: MFMA with fp32 accumulation; fp32: the exact
 * f32 MFMA (a k-ordered fmaf chain).  x [B,H,W,*] and y [B,2H,2W,*] are 16-byte aligned channel windows; Cin, Cout multiples of 8 up to 384
 * (EY_EUNSUPPORTED otherwise).  bias: DEVICE fp32 [Cout].  w_packed: ey_deconv2x2_pack_weight's output on the device, 16-byte aligned. */
size_t ey_deconv2x2_packed_bytes(int dtype, int Cin, int Cout);
/* HOST: w_iohw fp32 [Cin][Cout][2][2] (the nn.ConvTranspose2d layout) -> dst (dst_bytes >= ey_deconv2x2_packed_bytes). */
int ey_deconv2x2_pack_weight(int dtype, int Cin, int Cout, const float* w_iohw, void* dst, size_t dst_bytes);
int ey_deconv2x2(int dtype, int B, int H, int W, int Cin, int Cout, const void* x, int x_cstride, const void* w_packed, const float* bias, void* y,
                 int y_cstride, ey_stream_t stream);

/* ---- Segment validation: mask IoU (utils/metrics.py:137-153 mask_iou, with the ground-truth expansion of SegmentationValidator._process_batch,
 * models/yolo/segment/val.py:204-213), for every image of a batch in one call.  For image b with N_b predictions and M_b instances:
 *   inter[m][n] = #{pixels where gt m and prediction n are both set},  a_gt[m], a_pred[n] = #{set pixels}        exact integers
 *   iou[m][n]   = fl(inter / fl(fl(fl(a_gt + a_pred) - inter) + 1e-7f))                                           fp32, one rounding per op
 * (the reference's float matmul, sums and `union + eps`; no FMA contraction, IEEE division).  A union of 0 gives exactly 0.
 * pred: DEVICE uint8 [pred_off[B]][H][W], 0 = clear, anything else = set (what ey_process_mask writes), image b's rows are
 * pred_off[b] .. pred_off[b+1] - 1.  gt, by gt_mode:
 *   EY_MASK_GT_STACK  DEVICE uint8 [gt_off[B]][H][W] like pred (the reference's overlap_mask=False layout);
 *   EY_MASK_GT_INDEX  DEVICE int32 [B][H][W], instance m of image b = the pixels equal to m + 1 (overlap_mask=True: the reference repeats the
 *                     map M_b times and compares; here the map is read, never repeated).  M_b comes from gt_off -- an instance that was
 *                     painted over completely has area 0 -- and may exceed 255; other values (0, negative, > M_b) belong to no instance.
 * pred_off / gt_off (B + 1 entries, [0] == 0, non-decreasing) and out_off (B entries) are HOST arrays.  Image b's row-major [M_b][N_b] matrix is
 * written at iou + out_off[b] (and inter + out_off[b] when inter != NULL; int32); nothing else of iou / inter is touched, and an image
 * with N_b == 0 or M_b == 0 has no matrix (its out_off is ignored).  B == 0 is valid.  workspace: DEVICE, 16-byte aligned,
 * ey_mask_iou_workspace_bytes(H, W, pred_off[B], gt_off[B]) bytes: the bit-packed operands (64 pixels per word, one wave64 ballot each).
 * Three launches (pack predictions, pack ground truth, pairs), no atomics: the same bytes run to run.  EY_EUNSUPPORTED -- before anything
 * is launched -- for B > 128 or H * W > 2^24 (the areas must be exact in fp32); EY_EINVAL for bad arguments. */
enum { EY_MASK_GT_STACK = 0, EY_MASK_GT_INDEX = 1 };
size_t ey_mask_iou_workspace_bytes(int H, int W, long n_pred, long n_gt);
int ey_mask_iou(int gt_mode, int B, int H, int W, const uint8_t* pred, const int* pred_off, const void* gt, const int* gt_off, const long* out_off,
                float* iou, int* inter, void* workspace, size_t workspace_bytes, ey_stream_t stream);

/* ---- FastSAM prompt selection (ultralytics/models/fastsam/predict.py:61-103 FastSAMPredictor.prompt; the resize of utils/ops.py:716-737
 * scale_masks is folded in and never materialised).  For every image b of a batch, with M the N_b network-resolution masks of the image,
 * R(M) = F.interpolate(M[crop], (H0, W0), mode="bilinear", align_corners=False) and the prompts shared by all images (predict.py:75,86):
 *   full[n]     = sum of R(M_n)
 *   inter[p][n] = sum of R(M_n) over rows y1 <= y < min(y2, H0) and columns x1 <= x < min(x2, W0)                          (predict.py:80)
 *   iou[p][n]   = fl(inter / fl(fl(bbox_area_p + full) - inter)),  bbox_area_p = (y2 - y1)(x2 - x1) of the prompt as given     (predict.py:79-84)
 *   best[b][p]  = argmax_n iou[p][n] over the image's masks as an index INSIDE the image, ties to the lower index; -1 when N_b == 0
 *   hit[q][n]   = R(M_n)[y_q][x_q] != 0: a set pixel among the (up to) 2 x 2 sources of the point whose two weights are both not 0
 *   keep[n]     = (n is some box's best) | pk[n];  pk starts all 0 -- all 1 when Q > 0 and the labels sum to 0 -- and every point, in order,
 *                 writes (label != 0) into the masks it hits (predict.py:94-101).  Q == 0: pk = 0.
 * None of R(M) is stored: bilinear resizing is linear and separable, so a sum over a box is sum_ij M[i][j] Wy[i] Wx[j] with the per-axis weights
 * summed over the box's rows / columns; one pass over the mask bytes scores every box.  Per-axis source index and weights are torch's CPU
 * operator's, in fp32: in == out copies; otherwise r = max(fmaf((float)in / out, y + 0.5f, -0.5f), 0), i0 = min((int)r, in - 1),
 * l1 = clamp(r - i0, 0, 1), i1 = i0 + (i0 < in - 1), l0 = 1 - l1.  All sums are fp32 in a fixed order (csrc/fastsam.hip): a weight adds its
 * terms by ascending target coordinate; a thread adds Wx over the set bytes of a row inside one 16-byte word, then Wy times that row sum to its
 * accumulator, words ascending with a stride of 256; 64 lanes meet in an xor tree, 4 waves in order.  With original == mask size every weight
 * is 1 and the areas are exact integers.
 * masks: DEVICE uint8 [mask_off[B]][mh][mw], 0 = clear, anything else = set (what ey_process_mask writes); image b owns rows mask_off[b] ..
 * mask_off[b+1] - 1.  Every byte is read once.  HOST arrays: mask_off (B + 1 entries, [0] == 0, non-decreasing); geo [B][6] = top, bottom, left,
 * right, H0, W0: the crop rows top .. bottom - 1 and columns left .. right - 1 of scale_masks(padding=True) (gain = min(mh / H0, mw / W0),
 * pad = (m - orig * gain) / 2, top = int(pad_h), bottom = int(mh - pad_h), ...) and the target size; boxes [P][4] = x1, y1, x2, y2;
 * points [Q][2] = x, y; labels [Q].  P and Q may each be 0, not both.
 * Outputs (DEVICE): full fp32 [N], inter / iou fp32 [P][ld], hit uint8 [Q][ld], keep uint8 [N], best int32 [B][P], with N = mask_off[B] and
 * ld >= N the row stride; nothing else is written.  inter / iou / best may be NULL when P == 0, hit when Q == 0.  workspace: DEVICE, 16-byte
 * aligned, ey_mask_prompt_workspace_bytes(B, mh, mw, P) bytes (the weight tables).  Three launches (weights, scores, selection), no atomics: the
 * same bits run to run; graph-capturable.
 * EY_EINVAL: null pointers, a box with x2 <= x1 or y2 <= y1, negative coordinates, a point outside [0, W0) x [0, H0) of any image, a bad crop.
 *   This deviates from the reference, which for such prompts slices with Python's rules (predict.py:80: a negative coordinate counts from the
 *   far edge, an empty slice sums to 0) or raises an IndexError (predict.py:101); here they are refused.
 * EY_EUNSUPPORTED (before any launch): B > 64, P > 32, Q > 32, mh * mw > 2^24, a coordinate or target size above 32767 (the reference's
 *   int32 box area, predict.py:79), or weight tables (mh + mw) * slots(P) * 4 bytes above 156 KiB of LDS, slots = 2, 5, 17, 33 for P <= 1, 4, 16, 32. */
size_t ey_mask_prompt_workspace_bytes(int B, int mh, int mw, int P);
int ey_mask_prompt(int B, int mh, int mw, const uint8_t* masks, const int* mask_off, const int* geo, int P, const int* boxes, int Q, const int* points,
                   const int* labels, long ld, float* full, float* inter, float* iou, int* best, uint8_t* hit, uint8_t* keep, void* workspace,
                   size_t workspace_bytes, ey_stream_t stream);

/* ---- scale_masks (utils/ops.py:716-737): y[pl] = F.interpolate(x[pl][top:bottom, left:right], (H0, W0), mode="bilinear", align_corners=False)
 * for `planes` contiguous H x W planes, with the per-axis index and weights of ey_mask_prompt and
 *   y = fl(fl(l0y * fl(fl(l0x * a) + fl(l1x * b))) + fl(l1y * fl(fl(l0x * c) + fl(l1x * d))))        fp32, one rounding per operation.
 * in_dtype EY_MASK_U8 -> fp32 output; EY_F32 -> fp32; EY_F16 -> f16 (the fp32 value rounded once).  x, y: DEVICE, contiguous. */
enum { EY_MASK_U8 = 2 };
int ey_scale_masks(int in_dtype, long planes, int H, int W, int top, int bottom, int left, int right, int H0, int W0, const void* x, void* y, ey_stream_t stream);

/* ---- Object tracking (reference trackers/byte_tracker.py BYTETracker.update, trackers/utils/kalman_filter.py KalmanFilterXYAH,
 * trackers/utils/matching.py).  Definition, phases, resources and bounds: DESIGN.md section 7r; the text of both kernels is
 * csrc/track_core.inc.h, which also compiles for the host with one lane.
 *
 * ey_linear_assignment: B independent thresholded assignments in one launch, one workgroup each.  Problem b has an n x m fp32 cost matrix
 * with row stride ld (elements) and finds the partial matching M that minimises sum over M of (c_ij - thresh[b]); pairs with c_ij > thresh[b]
 * and NaN / Inf costs are never matched (what lap.lapjv(cost, extend_cost=True, cost_limit=thresh) computes).  Shortest augmenting paths with
 * fp64 duals; equal costs go to the lower column, a tie between matching and not matching to not matching; the same bits run to run.
 * desc: DEVICE int64 [B][4] = cost pointer, n, m, ld; n and m are clamped to 0 .. nmax / mmax.  thresh: DEVICE fp32 [B].
 * row_to_col: DEVICE int32 [B][ldr], entries 0 .. n-1 of row b are written (-1 = unmatched), nothing else; col_to_row: [B][ldc], entries
 * 0 .. m-1.  workspace: DEVICE, 16-byte aligned, ey_linear_assignment_workspace_bytes(B, nmax, mmax) bytes.  Loops: n augmentations of at most
 * n + 1 path steps, each one pass over the m columns. */
size_t ey_linear_assignment_workspace_bytes(int B, int nmax, int mmax);
int ey_linear_assignment(int B, const long* desc, const float* thresh, int nmax, int mmax, int* row_to_col, int ldr, int* col_to_row, int ldc,
                         void* workspace, size_t workspace_bytes, ey_stream_t stream);

/* ey_bytetrack_update: one ByteTrack frame for B independent streams in ONE launch, one workgroup per stream; the tracks live on the device.
 * rows: DEVICE fp32 [B][cap][6] = x1,y1,x2,y2,score,cls in image pixels; count: DEVICE int32 [B], clamped to 0 .. cap.  A stream whose count
 * is 0 is left alone bit for bit (only out_count[b] = 0 is written).  A row with a NaN / Inf coordinate or score is not a detection.
 * State, read and written in place (all zero = a fresh tracker): kf fp64 [B][max_tracks][72] = mean[8], covariance[8][8]; slot_i int32
 * [B][max_tracks][8] = state (0 free, 1 tracked, 2 lost), activated, id, idx, frame, start frame, tracklet_len, 0; slot_f fp32
 * [B][max_tracks][2] = score, cls; hdr int32 [B][4] = frame_id, last id given, overflow count, 0.  A new track takes the lowest free slot; a
 * slot freed by the unconfirmed round of a frame is free for the new tracks of the same frame, one freed by expiry or as a duplicate from
 * the next frame on.  With no free slot a new track is not started and hdr[2] counts it.
 * Outputs: out_rows fp32 [B][cap][8] = x1,y1,x2,y2 (fp32 of the fp64 posterior), id, score, cls, idx -- rows 0 .. out_count[b]-1, ascending
 * id, nothing else is written; out_ids int32 [B][cap]; out_count int32 [B].
 * workspace: DEVICE, 16-byte aligned, ey_bytetrack_workspace_bytes(B, cap, max_tracks) bytes, nothing in it survives the call.
 * EY_EUNSUPPORTED (nothing launched): 16 * max_tracks + 24 * cap > 65536 (the boxes of a stream are held in LDS). */
size_t ey_bytetrack_workspace_bytes(int B, int cap, int max_tracks);
int ey_bytetrack_update(int B, int cap, int max_tracks, float track_high_thresh, float track_low_thresh, float new_track_thresh, float match_thresh,
                        int max_time_lost, int fuse_score, const float* rows, const int* count, double* kf, int* slot_i, float* slot_f, int* hdr,
                        float* out_rows, int* out_ids, int* out_count, void* workspace, size_t workspace_bytes, ey_stream_t stream);

/* ---- Mask polygons (reference utils/ops.py:793-821 masks2segments: cv2.findContours(x, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) per mask).
 * ey_mask_contours: the external contours of n binary masks in ONE launch, one workgroup per mask: OpenCV's border following (Suzuki & Abe
 * 1985, algorithm 1), the raster scan for the next border start spread over the workgroup, each border followed by one lane in the
 * sequential order.  Definition, phases and bounds: DESIGN.md section 7s; the kernel's text is csrc/contours_core.inc.h, which also compiles for
 * the host with one lane.
 * masks: DEVICE uint8 [n][h][w], contiguous, non-zero = set; never written.  windows: DEVICE int32 [n][4] = x0, y0, x1, y1 or NULL: mask b is
 * scanned in columns x0 .. x1-1 and rows y0 .. y1-1 only (clamped to the mask) and everything outside counts as 0; with every set pixel
 * inside its window the result is that of the whole mask.
 * Outputs, per mask b: info int32 [n][4] = contours found, vertices found, flags (1: a capacity was too small, 2: a border walk passed its
 * step bound of 8 (h + 2)(w + 2) + 8), 0; lens int32 [n][contour_cap]: the vertex count of contour k in the order of discovery (OpenCV lists
 * them last found first); verts int32 [n][vertex_cap][2]: x, y of the vertices, contour after contour.  The counts in info are complete even
 * when a capacity was too small: nothing is written past lens[b][contour_cap) and verts[b][vertex_cap), flag 1 is set, and a second call with
 * the capacities info asks for gives the whole result.
 * workspace: DEVICE, 16-byte aligned, ey_mask_contours_workspace_bytes(n, h, w) bytes (one label per pixel and a frame), nothing in it
 * survives the call.  n == 0 launches nothing.  (h + 2)(w + 2) <= 2^30. */
size_t ey_mask_contours_workspace_bytes(int n, int h, int w);
int ey_mask_contours(int n, int h, int w, const uint8_t* masks, const int* windows, int contour_cap, int vertex_cap, int* lens, int* verts, int* info,
                     void* workspace, size_t workspace_bytes, ey_stream_t stream);

/* ---- Validation matching (csrc/match.hip; reference engine/validator.py:222-262 match_predictions and utils/metrics.py:326-382
 * ConfusionMatrix.process_batch).  ey_match_batch: the true positives of a batch's kept rows at T IoU thresholds and the batch's increments
 * of a confusion matrix in ONE launch, one workgroup per image, fp32, no host synchronisation (graph-capturable).  The closed forms, why
 * they equal the reference and the tie rules: csrc/match_core.inc.h (which also compiles for the host with one lane) and DESIGN.md 7t.
 * rows: DEVICE fp32 [B][max_det][stride >= 6] = x1,y1,x2,y2,conf,cls,... and count: DEVICE int32 [B], as the NMS entry points leave them;
 *   only columns 0..5 of the rows below count[b] (clamped to max_det) are read.  A row whose class is not in [0, nc) is skipped: its tp bytes
 *   are 0 and it adds nothing to the matrix.
 * xform: DEVICE fp32 [B][5] = padx, pady, gain, w0, h0 or NULL.  Given, every row's box goes through ops.scale_boxes + clip_boxes in registers
 *   (v - pad, IEEE division by gain, clamp to [0, w0] / [0, h0], the host path's fp32 operations in its order); NULL: the rows are in the
 *   labels' frame already.
 * gt: DEVICE fp32 [M][4] xyxy in original-image pixels; gt_cls: DEVICE int32 [M]; gt_off: HOST int32 [B+1] from 0, image b's labels are
 *   gt_off[b] .. gt_off[b+1]-1.  A label whose class is not in [0, nc) is skipped.
 * iou / iou_off / iou_ld (matrix mode): iou DEVICE fp32, iou_off HOST [B] element offsets, iou_ld HOST int32 [B]: image b's row-major
 *   [labels][iou_ld[b]] matrix starts at iou + iou_off[b] (images without labels have none); iou_ld[b] is the image's kept count as the host
 *   knows it, and no column at or beyond it is read whatever count[b] says.  Given, it replaces the box IoU (gt may be NULL) and xform is not used; with the
 *   box IoUs in it the outputs are identical to boxes mode.  NULL: box IoU = inter / ((a1 + a2) - inter + 1e-7f), no FMA contraction, IEEE
 *   division: metrics.box_iou bit for bit.
 * iouv: HOST fp32 [T], 1 <= T <= 16, compared in fp32 (>=).  cm_conf / cm_iou: only rows with conf > cm_conf take part in the matrix; a
 *   pair is a match when its IoU > cm_iou.
 * Outputs, either may be NULL: tp uint8 [B][max_det][T], rows at or beyond count[b] are left untouched; matrix int32 [(nc+1)^2], row =
 *   predicted class (nc = background), column = true class, accumulated with integer atomics (deterministic) and NOT zeroed by the call.
 * Exact IoU ties: among labels the higher label index wins, among detections the lower detection index.
 * The labels of an image, its takers (labels x T) and 12 bytes per row live in LDS: 1024 rows x 1024 labels x 16 thresholds fit (104 KiB of
 * the 160 KiB); past 160 KiB, or B > 128, the call returns EY_EUNSUPPORTED before anything is launched, with the limit named.  EY_EINVAL: null
 * required pointers, T outside 1..16, bad sizes or offsets.  A refusal leaves both outputs untouched. */
int ey_match_batch(int B, int max_det, int stride, const float* rows, const int* count, const float* xform, const float* gt, const int* gt_cls,
                   const int* gt_off, const float* iou, const long* iou_off, const int* iou_ld, int T, const float* iouv, int nc, float cm_conf, float cm_iou,
                   uint8_t* tp, int* matrix, ey_stream_t stream);

/* ---- K7 (module-level form): channel-slice copy with optional nearest x2 upsample — nn.Upsample / Concat
 * (conv.py:345-355) when they are not folded into the consuming conv.  dst[b,y,x,c] = src[b,y>>up,x>>up,c]. */
int ey_copy_nhwc(int dtype, int B, int H, int W, int C, int up, const void* src, int src_cstride, void* dst,
                 int dst_cstride, ey_stream_t stream);
/* NCHW-contiguous <-> NHWC view transposes (boundary with callers that hand over plain contiguous tensors). */
int ey_nchw_to_nhwc(int dtype, int B, int C, int H, int W, const void* src, void* dst, int dst_cstride, ey_stream_t stream);
int ey_nhwc_to_nchw(int dtype, int B, int C, int H, int W, const void* src, int src_cstride, void* dst, ey_stream_t stream);

/* ---- GPU pre-processing: LetterBox.__call__ (data/augment.py:1556-1591: cv2.resize INTER_LINEAR to
 * (new_h,new_w) + copyMakeBorder with 114) and BasePredictor.preprocess (engine/predictor.py:123-133: BGR->RGB,
 * HWC->CHW, uint8 -> f16/f32, /255) for ONE image, as one kernel.  src: device uint8 [src_h][src_w][3] (row pitch
 * src_row_bytes); dst: one [3][H][W] image slot of the NCHW batch tensor (out_dtype).  The caller computes the
 * LetterBox geometry (new size, top/left padding); the resize follows OpenCV's 8-bit fixed-point INTER_LINEAR path. */
int ey_letterbox(int out_dtype, const uint8_t* src_hwc, int src_h, int src_w, int src_row_bytes, void* dst_chw, int H, int W,
                 int new_h, int new_w, int top, int left, int pad_value, int swap_rb, ey_stream_t stream);
/* The same for B images of ONE shape in one launch (a decoded batch: image i at src_hwc + i * src_image_bytes -> slot i of the
 * [B][3][H][W] tensor; one geometry for all).  With new size == source size this is BasePredictor.preprocess alone: uint8 HWC BGR ->
 * RGB CHW /255 on the device, so a host batch crosses PCIe as 3 bytes per pixel instead of 6 (f16) or 12 (f32). */
int ey_letterbox_batch(int out_dtype, const uint8_t* src_hwc, int B, int src_h, int src_w, int src_row_bytes, long src_image_bytes,
                       void* dst_chw, int H, int W, int new_h, int new_w, int top, int left, int pad_value, int swap_rb,
                       ey_stream_t stream);

/* Linear copy as an ordinary kernel in `stream`: dst (device) <- src (device, or PINNED HOST memory that the device reads over PCIe
 * itself; a small persistent grid then).  The upload path of `YOLO.predict_batches`: on this stack an H2D hipMemcpyAsync does not
 * overlap with kernels of other streams, a kernel does.  nbytes and both pointers 16-byte aligned. */
int ey_copy_linear(const void* src, void* dst, size_t nbytes, ey_stream_t stream);

/* ---- K8a: linear attention core (LinearAttention.forward, block.py:3360-3373) between the qkv and proj convs.
 * qkv [B,N,3C] channel order [q(h0..)|k|v] (block.py:3364); y [B,N,C]:  k=softmax_d(k); q=softmax_N(q);
 * ctx_h = k_h^T v_h; y_h = q_h ctx_h.  head_dim = C/heads <= 64. */
int ey_linear_attention(int dtype, int B, int N, int C, int heads, const void* qkv, int qkv_cstride, void* y,
                        int y_cstride, ey_stream_t stream);

/* ---- K8b: softmax attention core (Attention.forward, block.py:1042-1053) of the YOLO11 baseline PSA block.
 * qkv [B,N,heads*(2*kd+hd)] per-head channel order [q(kd)|k(kd)|v(hd)]; y [B,N,heads*hd] = v @ softmax(q^T k * scale)^T. */
int ey_softmax_attention(int dtype, int B, int N, int heads, int kd, int hd, float scale, const void* qkv,
                         int qkv_cstride, void* y, int y_cstride, ey_stream_t stream);

/* ---- K8c: area attention core (AAttn.forward of YOLOv12's A2C2f, reference block.py:1313-1356).  q, k, v, y are [B,N,*] views
 * with their own channel strides; head h owns channels h*hd..h*hd+hd-1 of each (the qk conv's order [q: heads*hd | k: heads*hd],
 * block.py:1318-1319, 1332).  The N = H*W tokens of an image, in row-major order, are cut into `area` contiguous runs of N/area tokens
 * (block.py:1324-1327) and each (run, head) is attended separately:  y = softmax(q k^T * scale) v.  EY_EINVAL (nothing launched)
 * when N % area != 0, as the reference's reshape fails there.  f16 with hd = 32 (the only head_dim the YAMLs produce), 16-byte
 * aligned q/k/v and 8-byte aligned y: MFMA flash kernel with online softmax, any N/area >= 1.  Otherwise (fp32, other hd <= 64):
 * VALU kernel in fp32 (exact fp32 arithmetic for fp32 I/O), N/area <= 10176 (LDS).  Writes y only. */
int ey_area_attention(int dtype, int B, int N, int area, int heads, int hd, float scale, const void* q, int q_cstride, const void* k,
                      int k_cstride, const void* v, int v_cstride, void* y, int y_cstride, ey_stream_t stream);

/* ---- K8d: softmax attention over ALL tokens of an image, the core of GlobalSparseAttn.forward of the LGL block (reference
 * block.py:3147-3152: attn = softmax(q k^T * scale); y = attn v).  Views as ey_area_attention with one area: q, k, v, y [B,N,*] with their
 * own channel strides, head h owns channels h*hd..h*hd+hd-1 (the qkv Linear's order [q: heads*hd | k | v], block.py:3148).
 * f16 with hd in {16, 32, 64}, 16-byte aligned q/k/v (cstrides multiples of 8) and 8-byte aligned y: MFMA flash kernel, online softmax
 * with fp32 statistics, any N >= 1 at a fixed 2 x 64 x (hd + 8) f16 of LDS; keys past N are masked to -inf, queries past N are not
 * stored.  Otherwise (fp32, unaligned views, other hd <= 64): the fp32 VALU kernel of ey_area_attention, N <= 10176 (its score rows
 * live in LDS); more tokens -> EY_EUNSUPPORTED, nothing launched.  Writes y only. */
int ey_flash_attention(int dtype, int B, int N, int heads, int hd, float scale, const void* q, int q_cstride, const void* k, int k_cstride,
                       const void* v, int v_cstride, void* y, int y_cstride, ey_stream_t stream);

/* Kernel the last ey_linear_attention / ey_softmax_attention / ey_area_attention / ey_flash_attention on this thread launched (tests); 0 = nothing launched.
 * Flash: EY_ATTN_FLASH_MFMA + hd (flash_attn_kernel<hd>, hd = 16, 32, 64; a group is an image), EY_ATTN_FLASH_F32 / _F16 (area_attn_kernel<T>, fp32 VALU).
 * Linear: EY_ATTN_LIN_F32 / _F16 (linattn_kernel<T>, fp32 VALU), EY_ATTN_LIN_MFMA (linattn_mfma_kernel).
 * Softmax VALU: EY_ATTN_SOFT_VALU + 4 (f16) + 2 (K staged in LDS: K_LDS) + 1 (nsplit == 1: one query block per (image, head)).
 * Softmax MFMA: EY_ATTN_SOFT_MFMA + NKS (softattn_mfma_kernel<NKS>, NKS = 4, 8, 10, 13).
 * Area: EY_ATTN_AREA_F32 / _F16 (area_attn_kernel<T>, fp32 VALU), EY_ATTN_AREA_MFMA (flash_attn_kernel<32>; a group is a run of an image). */
enum { EY_ATTN_LIN_F32 = 101, EY_ATTN_LIN_F16 = 102, EY_ATTN_LIN_MFMA = 103, EY_ATTN_SOFT_VALU = 200, EY_ATTN_SOFT_MFMA = 300,
       EY_ATTN_AREA_F32 = 401, EY_ATTN_AREA_F16 = 402, EY_ATTN_AREA_MFMA = 403,
       EY_ATTN_FLASH_MFMA = 500, EY_ATTN_FLASH_F32 = 501, EY_ATTN_FLASH_F16 = 502 };
int ey_attention_last_variant(void);

/* ---- K9+K10: DGQP quality + DFL expectation + anchor decode + score modulation for ONE pyramid level.
 * Detect._inference (head.py:117-148), DFL (block.py:87-90), make_anchors/dist2bbox (utils/tal.py:333-357),
 * GF2Detect._compute_quality_from_logits / _inference_with_quality (head.py:227-243,301-345).
 * box [B,H,W,4*16], cls [B,H,W,nc]; q_* = reg_conf weights (fp32, device) or NULL for plain Detect:
 *   q_w1 [64][20], q_b1 [64], q_w2 [64], q_b2 [1].
 * pred fp32 [B, 4+nc, A_total]; this level fills anchors [a_off, a_off + H*W). */
int ey_head_decode(int dtype, int B, int H, int W, int nc, float stride, const void* box, int box_cstride,
                   const void* cls, int cls_cstride, const float* q_w1, const float* q_b1, const float* q_w2,
                   const float* q_b2, int q_hidden, float* pred, int A_total, int a_off, ey_stream_t stream);

/* All pyramid levels of one head in ONE launch (arrays of length nlevels <= 4; same nc / q_hidden for every level; q_* arrays
 * NULL or holding NULLs for plain Detect).  Same arithmetic as ey_head_decode per level: Detect.forward decodes every level
 * after all towers ran (head.py:84-90,117-148), so the three small launches collapse into one grid that fills the chip. */
int ey_head_decode_levels(int dtype, int B, int nlevels, const int* H, const int* W, const float* stride, const void* const* box,
                          const int* box_cstride, const void* const* cls, const int* cls_cstride, int nc, const float* const* q_w1,
                          const float* const* q_b1, const float* const* q_w2, const float* const* q_b2, int q_hidden, float* pred,
                          int A_total, const int* a_off, ey_stream_t stream);

/* K9+K10 with the NMS candidate build fused in (predict mode, single label; Detect._inference head.py:117-148 followed by the
 * candidate selection of non_max_suppression, utils/ops.py:253,273-275): same arithmetic as ey_head_decode_levels, and per anchor the
 * best class (first maximal index), the sort key (score_bits << 32 | ~anchor) when score > conf_thres and the class passes
 * class_mask (else 0), and the box (cx,cy,w,h) go to `candidates` (ey_nms_candidates_bytes(B, A_total) bytes, 16-byte aligned):
 * exactly what ey_nms derives from `pred`, from the same fp32 values -- so ey_nms_candidates() returns bit-identical rows without the
 * (B,4+nc,A) tensor being written or re-read.  pred_or_null: also write the reference-layout prediction tensor (callers that want it).
 * The levels must cover all A_total anchors. */
size_t ey_nms_candidates_bytes(int B, int A);
int ey_head_decode_levels_nms(int dtype, int B, int nlevels, const int* H, const int* W, const float* stride, const void* const* box, const int* box_cstride,
                              const void* const* cls, const int* cls_cstride, int nc, const float* const* q_w1, const float* const* q_b1,
                              const float* const* q_w2, const float* const* q_b2, int q_hidden, float* pred_or_null, int A_total, const int* a_off,
                              float conf_thres, const uint8_t* class_mask, void* candidates, size_t candidates_bytes, ey_stream_t stream);
/* ey_head_decode_levels_nms with the towers' closing 1x1 convs inside the decode kernel (predict mode: nothing else reads their
 * logits) -- replaces, per level, nn.Conv2d(64, 64, 1) of the box tower and Conv(c3, c3, 1) + SiLU -> nn.Conv2d(c3, nc, 1) of the
 * class tower (ultralytics/nn/modules/head.py:61,68-70) in front of the decode (:227-243,341-345).  Same candidates and pred, bit for
 * bit, as ey_conv2d (ACT_NONE) + ey_conv_pw_chain (SiLU, NONE) + ey_head_decode_levels_nms on the same tensors.
 *   box_feat[l]: (B, box_cin, H, W) output of cv2[l][1];  box_w[l] / box_b[l]: ey_conv_pack_weight(EY_F16, box_cout, box_cin, 1) / bias.
 *   fuse_cls = 1: cls[l] = (B, cls_cin[l], H, W) output of the tower's second DWConv; cls_w1 = ey_conv_pack_weight(EY_F16, cls_cmid,
 *     cls_cin[l], 1), cls_w2 = ey_conv_pack_weight(EY_F16, nc, ey_conv_chain_klen(cls_cmid), 1) of the column-permuted weights (as
 *     ey_conv_pw_chain), cls_b1 / cls_b2 the fp32 biases (all required).
 *   fuse_cls = 0: cls[l] = the (B, nc, H, W) class logits; the cls_* weight arguments are ignored (may be NULL).
 * Shape gate -- f16, <= 4 levels, box_cin == box_cout == 64, cls_cin in 72..96 (% 8), cls_cmid == 80, nc % 8 == 0 and 64 < nc <= 80,
 * every view 16-byte aligned: EY_EUNSUPPORTED before anything is launched otherwise; all levels of a call are fused, or none.
 * Variant code (ey_head_decode_last_variant): EY_HD_TAIL_BOX or EY_HD_TAIL_BOX_CLS (+ EY_HD_QUALITY) + EY_HD_NMS. */
int ey_head_tail_decode_levels_nms(int dtype, int B, int nlevels, const int* H, const int* W, const float* stride, const void* const* box_feat,
                                   const int* box_cstride, int box_cin, int box_cout, const void* const* box_w, const float* const* box_b,
                                   const void* const* cls, const int* cls_cstride, int fuse_cls, const int* cls_cin, int cls_cmid,
                                   const void* const* cls_w1, const float* const* cls_b1, const void* const* cls_w2, const float* const* cls_b2, int nc,
                                   const float* const* q_w1, const float* const* q_b1, const float* const* q_w2, const float* const* q_b2, int q_hidden,
                                   float* pred_or_null, int A_total, const int* a_off, float conf_thres, const uint8_t* class_mask, void* candidates,
                                   size_t candidates_bytes, ey_stream_t stream);
/* Second half of ey_nms (selection + greedy suppression, utils/ops.py:277-309 + torchvision.ops.nms) on a candidate buffer
 * written by ey_head_decode_levels_nms.  Outputs as ey_nms.  The tail of the buffer (beyond keys / class ids / boxes) is the scratch of
 * the predict-mode fast path (sorted candidate records + the pairwise suppression bit matrix) and is written by this call. */
int ey_nms_candidates(int B, int nc, int A, void* candidates, size_t candidates_bytes, float iou_thres, int max_det, int max_nms, float max_wh,
                      int agnostic, float* out_boxes, int32_t* out_count, int32_t* out_index, ey_stream_t stream);

/* ---- End2end (NMS-free) heads: E2EDetect = GF2Detect with end2end=True (head.py:273-298,799-824).
 * ey_head_decode_levels_xyxy: ey_head_decode_levels with rows 0-3 of pred = x1,y1,x2,y2 in input pixels (Detect.decode_bboxes passes
 *   xywh = not end2end to dist2bbox, head.py:163-165, utils/tal.py:348-357); rows 4.. unchanged.
 * ey_e2e_topk: Detect.postprocess (head.py:167-189) on that tensor: out_rows [B, k, 6] fp32 = the k best (anchor, class) pairs of each
 *   image in descending score order, row = x1,y1,x2,y2,score,class; k = min(max_det, A) is the caller's; out_index [B, k] (anchor of
 *   each row) or NULL.  Equal scores: lower anchor, then lower class first (torch.topk leaves that order unspecified).
 *   1 <= k <= min(A, 1611): the LDS bound of the selection workgroup, see ey_nms.
 *   workspace: ey_e2e_topk_workspace_bytes(B, nc, A) bytes, 16-byte aligned. */
int ey_head_decode_levels_xyxy(int dtype, int B, int nlevels, const int* H, const int* W, const float* stride, const void* const* box,
                               const int* box_cstride, const void* const* cls, const int* cls_cstride, int nc, const float* const* q_w1,
                               const float* const* q_b1, const float* const* q_w2, const float* const* q_b2, int q_hidden, float* pred,
                               int A_total, const int* a_off, ey_stream_t stream);
size_t ey_e2e_topk_workspace_bytes(int B, int nc, int A);
int ey_e2e_topk(int B, int nc, int A, const float* pred_xyxy, int k, float* out_rows, int32_t* out_index, void* workspace,
                size_t workspace_bytes, ey_stream_t stream);

/* Form of head_decode_kernel the last ey_head_decode* on this thread launched (tests); 0 = nothing launched.
 * EY_HD_VEC (16-byte staging: nc % 8 == 0, aligned views) or EY_HD_SCALAR, + EY_HD_QUALITY (DGQP quality head) + EY_HD_NMS (fused
 * NMS candidates).  head_tail_decode_kernel (ey_head_tail_decode_levels_nms): EY_HD_TAIL_BOX (box tail inside) or EY_HD_TAIL_BOX_CLS
 * (box tail and class chain inside) in place of VEC / SCALAR. */
enum { EY_HD_VEC = 1, EY_HD_SCALAR = 2, EY_HD_TAIL_BOX = 3, EY_HD_TAIL_BOX_CLS = 4, EY_HD_QUALITY = 10, EY_HD_NMS = 100 };
int ey_head_decode_last_variant(void);

/* ---- Block programs: a chain of layers on SMALL feature maps (<= 4096 pixels per image; built for the 20x20 part of the network at
 * 640x640: stride-2 Conv -> DSC3K2_Wavelet -> SPPF -> C2PSA_LinearAttention, nn/modules/block.py:204-223,3412-3497,3749-3788; the
 * last neck block; the 20x20 Detect towers, head.py:59-70) executed by ONE launch: one persistent 1024-thread workgroup per image
 * walks the stages below with a workgroup barrier between them.  Each stage is one of the operators above with the same
 * arithmetic (f16 storage between stages, fp32 accumulate); f16 only.
 *
 * A tensor reference is (addr, ext): ext < 0 -> addr is an absolute device pointer (weights, intermediates owned by the caller for
 * the life of the program); ext >= 0 -> addr is a BYTE offset into the ext-th external tensor handed to ey_block_run (the chain's
 * inputs and outputs, which change from call to call).  *_img = elements between consecutive images of that tensor; *_cs = pixel
 * stride (elements) as everywhere in this ABI. */
enum { EY_BLK_CONV = 0, EY_BLK_DW = 1, EY_BLK_DWT = 2, EY_BLK_POOL = 3, EY_BLK_LINATTN = 4 };
typedef struct {
  int32_t op;
  int32_t H, W, Ho, Wo;        /* input / output extent of the stage */
  int32_t k, stride, act;      /* CONV: k in {1,3}, stride in {1,2}, pad k/2.  DW: k in {3,5,7}, stride 1 */
  int32_t nsrc;                /* CONV: 1 or 2 virtually concatenated sources; others: 1 */
  int64_t src[2]; int32_t src_ext[2]; int64_t src_img[2]; int32_t src_cs[2]; int32_t src_C[2];
  const void* w;               /* CONV: ey_conv_pack_weight layout (group sets w_g elements apart); DW: [k][k][C] f16 */
  const float* bias;           /* CONV: [sets][Cout] fp32 or NULL; DW: [C] fp32 or NULL */
  int64_t w_g; int32_t w_gmax;
  int64_t y; int32_t y_ext; int64_t y_img; int32_t y_cs; int32_t Cout;   /* POOL: y = the y1 slot (y2, y3 follow at C-channel steps); LINATTN: Cout = C */
  int32_t has_res; int64_t res; int32_t res_ext; int64_t res_img; int32_t res_cs;
  int32_t has_addz; int64_t addz; int32_t addz_ext; int64_t addz_img; int32_t addz_cs, addz_H, addz_W;
  float out_scale;
  int32_t ngroup; int64_t src_g, y_g;   /* CONV: channel-offset groups as in ey_conv_desc */
  int32_t heads;               /* LINATTN: heads of 64 channels, even */
  /* filled by ey_block_compile */
  int32_t kpad, nt_pack, mt, nti, lds, tile_nti;
  int32_t tile_src_lds[2], tile_src_lcs[2], tile_y_lds, tile_y_lcs, tile_res_lds, tile_res_lcs, tile_lds_bytes;  /* pointwise-chain LDS placement */
  float zsy, zsx;
} ey_block_stage;
size_t ey_block_stage_sizeof(void);
size_t ey_block_program_bytes(int nstages);
/* host -> host: validate + derive; upload `out_host` (ey_block_program_bytes bytes) to the device afterwards. */
int ey_block_compile(const ey_block_stage* stages_host, int nstages, void* out_host, size_t out_bytes);
/* One launch: grid = B workgroups.  ext_ptrs_host: the `next` (<= 8) external tensors' device base pointers (host array, read at call time). */
int ey_block_run(const void* program_dev, int nstages, int B, const void* const* ext_ptrs_host, int next, ey_stream_t stream);
/* Pointwise chains: when every stage is a 1x1 / stride-1 / single-group conv on one map (ey_block_tileable(compiled program) != 0) the
 * pixels do not interact, and the program runs as one 256-thread workgroup per 32-pixel tile (grid = tiles x B: the whole chip) instead
 * of one workgroup per image, chain-internal tensors in LDS: C2PSA's proj -> ffn -> ffn -> cv2, cv1 -> qkv, DSC3k's cv3 -> cv2 (block.py:3412-3497,1506-1562). */
int ey_block_tileable(const ey_block_stage* compiled_host, int nstages);
int ey_block_run_tiles(const void* program_dev, int nstages, int B, int H, int W, int lds_bytes /* compiled stage 0's tile_lds_bytes */,
                       const void* const* ext_ptrs_host, int next, ey_stream_t stream);
/* Register-weight executor for the same programs (block_chain_kernel): one 512-thread workgroup per 64 consecutive pixels of an image
 * (grid = ceil(H*W/64) x B); in every stage a wave keeps the weight fragments of ITS 16-row output blocks in registers (requested at
 * kernel start / while the stage before multiplies), every global source, residual and bias goes to LDS once before the first
 * barrier, one LDS-only barrier per stage.  Same arithmetic, byte-equal results.
 * ey_block_fast_plan: pure host function of a COMPILED program; returns 1 and fills plan_host (ey_block_fast_plan_bytes() bytes, host
 * memory, position-independent: keep it beside the program) when the program is eligible, 0 otherwise.  Eligible = tileable, at most
 * 4 stages, no addz, source channels multiples of 32, Cout a multiple of its packed block tile (16 * nt_pack) and <= 512, the list of
 * (k-steps, row blocks per wave) per stage is one the kernel is instantiated for (the per-wave fragment budget; C2PSA's head and tail
 * at c = 64 / 128), no stage writes in place over one of its own sources, at most 4096 16-byte vectors of global inputs per tile,
 * and the LDS plan (dead tensors aliased) fits 96 KiB.
 * ey_block_run_chain = ey_block_run_tiles plus the plan (NULL = none): with a plan and the tunable chain_fast != 0 it launches the
 * register-weight executor, otherwise block_tile_kernel.  ey_block_last_variant: the executor the last ey_block_run* call on this thread took. */
enum { EY_BLK_RAN_IMAGE = 1, EY_BLK_RAN_TILE = 2, EY_BLK_RAN_CHAIN = 3 };
size_t ey_block_fast_plan_bytes(void);
int ey_block_fast_plan(const ey_block_stage* compiled_host, int nstages, void* plan_host, size_t plan_bytes);
int ey_block_run_chain(const void* program_dev, int nstages, int B, int H, int W, int lds_bytes, const void* plan_host,
                       const void* const* ext_ptrs_host, int next, ey_stream_t stream);
int ey_block_last_variant(void);
/* Developer tool: the same launch; workgroup 0 also stores wall_clock64() (100 MHz ticks) at the start and after every stage into
 * tstamps_dev[nstages + 1] (tools/block_stage_times.py prints the per-stage split). */
int ey_block_run_timed(const void* program_dev, int nstages, int B, const void* const* ext_ptrs_host, int next, long long* tstamps_dev, ey_stream_t stream);

/* ---- K11: batched per-image NMS (non_max_suppression, utils/ops.py:230-316, and the torchvision.ops.nms it calls
 * at :296).  multi_label=0: best class per anchor (predict, ops.py:273-275); multi_label=1: one candidate per
 * (anchor, class) pair above conf (validation, ops.py:270-272; needs the _ml workspace).
 * pred fp32 [B,4+nc,A] (xywh + scores), NOT modified.
 * out_boxes fp32 [B,max_det,6] = x1,y1,x2,y2,conf,cls in kept (descending score) order; out_count int32 [B];
 * out_index int32 [B,max_det] = anchor index of each kept row (may be NULL); class_mask uint8 [nc] or NULL
 * (the `classes=` filter).  workspace: ey_nms_workspace_bytes(B, A) bytes.
 * max_det (ey_nms, ey_nms_candidates) and k (ey_e2e_topk) are bounded by the LDS of the one workgroup that selects an image: its fixed
 * state (82416 B) plus, per kept box, the class-offset box, the result row and the index (48 B; 80 B with the per-owner rank lists of
 * the class-partitioned greedy, which only runs for max_det <= 512) plus 4096 B of reserve must fit 160 KiB, i.e.
 * 82416 + 48 * max_det + 4096 <= 163840: 1 <= max_det <= 1611.  From 1612 up the call returns EY_EINVAL ("nms: max_det=1612 needs
 * 159792 B of LDS") before the selection is launched; nothing is written to the outputs. */
size_t ey_nms_workspace_bytes(int B, int A);
size_t ey_nms_workspace_bytes_ml(int B, int nc, int A);
int ey_nms(int B, int nc, int A, const float* pred, float conf_thres, float iou_thres, int max_det, int max_nms,
           float max_wh, int agnostic, int multi_label, const uint8_t* class_mask, float* out_boxes, int32_t* out_count,
           int32_t* out_index, void* workspace, size_t workspace_bytes, ey_stream_t stream);

/* ---- Oriented boxes (csrc/obb.hip).
 * ey_obb_decode_levels: eval-mode OBB head (ultralytics/nn/modules/head.py:383-399 with Detect._inference :117-148, DFL block.py:87-90,
 *   dist2rbox utils/tal.py:366-385) for up to 4 pyramid levels in ONE launch.  Per level NHWC maps of `dtype`: box [B,H,W,64] logits,
 *   cls [B,H,W,nc] logits, angle [B,H,W,1] logits, each with its pixel stride.  pred fp32 [B, 4+nc+1, A_total]: rows 0-3 = the rotated box
 *   (cx, cy, w, h) * stride, rows 4.. = sigmoid(cls), last row = the angle (sigmoid(a) - 0.25) * pi, unscaled.
 * ey_probiou: utils/metrics.py::batch_probiou (:244-275, eps = 1e-7): obb1 [N,5], obb2 [M,5] xywhr fp32 -> out [N,M] fp32.
 * ey_nms_rotated: non_max_suppression(rotated=True) in single-label mode (utils/ops.py:230-297 with nms_rotated :146-164: fast-NMS on
 *   ProbIoU).  pred fp32 [B, 4+nc+1, A] as written by ey_obb_decode_levels, NOT modified.  Candidates: best class score > conf_thres
 *   (strict; conf_thres >= 0, EY_EINVAL otherwise) and class_mask (uint8 [nc] or NULL); the max_nms best by score, ordered by descending score, equal scores by ascending
 *   anchor; pair input (x + c max_wh, y + c max_wh, w, h, r), c = class (0 when agnostic), summed in fp32; column j is kept iff
 *   max(0, max_{i before j} probiou(i, j)) < iou_thres.  out_rows fp32 [B,max_det,7] = x,y,w,h,conf,cls,angle copied from pred, the first
 *   max_det kept columns in score order (zeros beyond the count); out_count int32 [B]; out_index int32 [B,max_det] = anchor of each row, -1
 *   beyond the count (may be NULL).  workspace: ey_nms_rotated_workspace_bytes(B, A, max_nms) bytes, 256-byte aligned.  No host
 *   synchronisation, no allocation: graph-capturable.  Exact at every candidate count up to max_nms.
 * ey_nms_rotated_ml: the same call in the validation regime, non_max_suppression(multi_label=True, rotated=True) (utils/ops.py:270-297):
 *   a candidate is every (anchor a, class c) with pred[4+c][a] > conf_thres (strict) and class_mask[c], up to A*nc per image (A*nc < 2^31),
 *   so one anchor can give several rows that share the box and the angle.  Order: descending score, equal scores by ascending a*nc + c
 *   (a stable sort of the reference's torch.where order; the reference's own argsort leaves ties unspecified).  The max_nms best go
 *   through the pair and keep stages of ey_nms_rotated, with the same fp32 expressions.  The max_nms-th score is found by a radix select
 *   over the key bits: no step ranks all A*nc candidates against each other.  Outputs as for ey_nms_rotated (out_index = anchor; the class
 *   is in column 5 of the row).  workspace: ey_nms_rotated_ml_workspace_bytes(B, nc, A, max_nms) bytes (0 for arguments the call refuses),
 *   256-byte aligned.  No host synchronisation, no float atomics: graph-capturable, the same bytes run to run.  nc == 1 is ey_nms_rotated's
 *   result.
 * ey_probiou_batch: batch_probiou(gt_b, pred_b) for every image of a batch in ONE launch.  pred fp32 [pred_off[B]][5], gt fp32
 *   [gt_off[B]][5] xywhr; pred_off / gt_off (B+1 entries from 0) and out_off (B entries, in elements) are HOST arrays as for ey_kpt_iou.
 *   Image b's row-major [M_b][N_b] matrix (ground truth x prediction) goes to out + out_off[b], bit-identical to ey_probiou(M_b, N_b, gt_b,
 *   pred_b); images with M_b == 0 or N_b == 0 have none; B == 0 is valid; B <= 128, otherwise EY_EUNSUPPORTED. */
int ey_obb_decode_levels(int dtype, int B, int nlevels, const int* H, const int* W, const float* stride, const void* const* box, const int* box_cstride,
                         const void* const* cls, const int* cls_cstride, const void* const* angle, const int* angle_cstride, int nc, float* pred,
                         int A_total, const int* a_off, ey_stream_t stream);
int ey_probiou(int N, int M, const float* obb1, const float* obb2, float* out, ey_stream_t stream);
size_t ey_nms_rotated_workspace_bytes(int B, int A, int max_nms);
int ey_nms_rotated(int B, int nc, int A, const float* pred, float conf_thres, float iou_thres, int max_det, int max_nms, float max_wh, int agnostic,
                   const uint8_t* class_mask, float* out_rows, int32_t* out_count, int32_t* out_index, void* workspace, size_t workspace_bytes,
                   ey_stream_t stream);
size_t ey_nms_rotated_ml_workspace_bytes(int B, int nc, int A, int max_nms);
int ey_nms_rotated_ml(int B, int nc, int A, const float* pred, float conf_thres, float iou_thres, int max_det, int max_nms, float max_wh, int agnostic,
                      const uint8_t* class_mask, float* out_rows, int32_t* out_count, int32_t* out_index, void* workspace, size_t workspace_bytes,
                      ey_stream_t stream);
int ey_probiou_batch(int B, const float* pred, const int* pred_off, const float* gt, const int* gt_off, float* out, const long* out_off, ey_stream_t stream);

/* ---- Pose estimation (csrc/pose.hip).  Levels are described as for ey_obb_decode_levels: per level an NHWC map kpt [B,H,W,nkpt*ndim] of
 *   `dtype` (logits of the cv4 towers) with its pixel stride, the level's stride and its first anchor a_off.  ndim is 2 (x, y) or 3
 *   (x, y, visibility), nkpt*ndim <= 256, 1 to 4 levels: anything else is EY_EUNSUPPORTED before any launch.  Windows that are not 16-byte
 *   aligned are read with scalar loads.
 * ey_kpts_decode_levels: Pose.kpts_decode (ultralytics/nn/modules/head.py:446-451) for every level in ONE launch.  out fp32: rows
 *   [nkpt*ndim][A_total] per image, images out_bstride elements apart (so it can write rows 4+nc.. of the prediction tensor in place).
 *   Anchor with grid cell (gx, gy): x = (v*2 + gx) * stride, y = (v*2 + gy) * stride -- one rounding, bit for bit the reference's fp32
 *   (v*2.0 + (anchor - 0.5)) * stride -- and sigmoid(v) for the third value.
 * ey_kpts_decode_rows: the same decode for the rows NMS kept.  index int32 [B,max_det] = anchor of each row (as ey_nms / the candidate
 *   NMS write it), count int32 [B]; out fp32 [B,max_det,nkpt,ndim].  Row r < count[b] with 0 <= index < A_total inside a level: that
 *   pixel's channels, bit-identical to ey_kpts_decode_levels; every other row (beyond the count, negative index, index outside every level:
 *   checked in the kernel before an address is formed) is zeros.  No host synchronisation, no allocation, no atomics: graph-capturable
 *   and the same bytes run to run.
 * ey_kpt_iou: utils/metrics.py::kpt_iou (:156-175, eps = 1e-7) for every image of a batch in ONE launch.  gt fp32 [gt_off[B]][K][3],
 *   area fp32 [gt_off[B]], pred fp32 [pred_off[B]][K][ndim] (x and y are read), sigma fp32 [K]; pred_off / gt_off (B+1 entries from 0) and
 *   out_off (B entries, in elements) are HOST arrays as for ey_mask_iou.  Image b's row-major [M_b][N_b] matrix (ground truth x prediction)
 *   goes to out + out_off[b]; nothing else is written; images with M_b == 0 or N_b == 0 have none; B == 0 is valid.  fp32 in the reference's
 *   order: d = dx^2 + dy^2, e = d / ((2 sigma)^2 * (area + eps) * 2), sum_k exp(-e) * (gt_v != 0) / (#visible + eps); a ground truth without a
 *   visible keypoint gives exactly 0.  K <= 64, B <= 128, otherwise EY_EUNSUPPORTED. */
int ey_kpts_decode_levels(int dtype, int B, int nlevels, const int* H, const int* W, const float* stride, const void* const* kpt, const int* kpt_cstride,
                          int nkpt, int ndim, float* out, long out_bstride, int A_total, const int* a_off, ey_stream_t stream);
int ey_kpts_decode_rows(int dtype, int B, int nlevels, const int* H, const int* W, const float* stride, const void* const* kpt, const int* kpt_cstride,
                        int nkpt, int ndim, int A_total, const int* a_off, int max_det, const int32_t* index, const int32_t* count, float* out,
                        ey_stream_t stream);
int ey_kpt_iou(int B, int K, int ndim, const float* pred, const int* pred_off, const float* gt, const int* gt_off, const float* area, const float* sigma,
               const long* out_off, float* out, ey_stream_t stream);

/* ---- Image classification (csrc/classify.hip).
 * ey_classify_pool: Classify.conv + AdaptiveAvgPool2d(1) + flatten (ultralytics/nn/modules/head.py:463-472) in ONE launch:
 *   out[b][co] = ( sum_p act( bias[co] + sum_ci x[b][p][ci] * w[co][ci] ) ) / (float)HW        p over the HW pixels of image b
 *   x: NHWC window [B, HW, *] of `dtype` with pixel stride x_cstride >= C1 (only the C1 channels are read; a window that is not 16-byte
 *   aligned is read with scalar loads); w: DEVICE [Cout][C1] in `dtype`, 16-byte aligned (the BN-folded 1x1 weight, row-major); bias: DEVICE
 *   fp32 [Cout]; out: DEVICE fp32 [B][Cout].  The (B, Cout, H, W) map is never written.  f16: MFMA with fp32 accumulation, Cout a multiple of
 *   16; fp32: a k-ordered fmaf chain per output, any Cout.  Any HW >= 1 (pixel tiles accumulate the per-channel sums of the activated values
 *   in fp32; the mean is that sum followed by one IEEE division), C1 a multiple of 8 up to 4096 (f16 above 2016: a pixel tile of more than 64 KiB
 *   of dynamic LDS; up to 2016 the launch is what it always was): EY_EUNSUPPORTED before any launch otherwise.
 * ey_classify_linear_softmax: Classify.linear + softmax(1) (head.py:472-475) + the top-min(nc, 5) classes in ONE launch, all outputs of fixed
 *   size (graph-capturable, no atomics, the same bytes run to run).  pooled: DEVICE fp32 [B][K]; w: DEVICE [nc][K] in `dtype`, 16-byte aligned;
 *   bias fp32 [nc].  logits / probs: fp32 [B][nc] (accumulation and everything behind it in fp32; softmax subtracts the row maximum);
 *   topk_index int32 / topk_prob fp32 [B][min(nc, 5)]: classes by descending probability, EQUAL PROBABILITIES BY ASCENDING CLASS INDEX (the
 *   reference's argsort is not stable; this is the rule here).  A row whose probabilities are NaN gets index -1, probability 0.
 *   1 <= nc <= 8192 and K a multiple of 8 up to 4096: EY_EUNSUPPORTED before any launch otherwise.
 * ey_classify_transform: classify_transforms(size) of the reference (ultralytics/data/augment.py:2346: torchvision Resize(S) ->
 *   CenterCrop(S) -> ToTensor, mean 0, std 1, crop fraction 1) for B uint8 HWC images of ONE shape (image i at src_hwc + i * src_image_bytes)
 *   -> [B][3][S][S] of out_dtype in [0, 1], channels reversed when swap_rb (BGR -> RGB).  Resized size: shorter side S, longer side
 *   int(S * long / short); crop origin int(round((n - S) / 2.0)) with round-half-to-even; filter: Pillow's antialiased BILINEAR per axis
 *   (scale = in / out, fs = max(scale, 1), center = (i + 0.5) scale, taps [max(int(center - fs + 0.5), 0), min(int(center + fs + 0.5), in)),
 *   weight max(0, 1 - |(x - center + 0.5) / fs|) normalised to sum 1), both axes applied in one pass with fp32 pixel sums and no uint8
 *   intermediate; only the pixels inside the crop are computed. */
int ey_classify_pool(int dtype, int B, int HW, int C1, int Cout, int act, const void* x, int x_cstride, const void* w, const float* bias, float* out,
                     ey_stream_t stream);
int ey_classify_linear_softmax(int dtype, int B, int K, int nc, const float* pooled, const void* w, const float* bias, float* logits, float* probs,
                               int32_t* topk_index, float* topk_prob, ey_stream_t stream);
int ey_classify_transform(int out_dtype, const uint8_t* src_hwc, int B, int src_h, int src_w, int src_row_bytes, long src_image_bytes, void* dst_chw, int S,
                          int swap_rb, ey_stream_t stream);

/* ---- Test-time augmentation (DetectionModel._predict_augment, nn/tasks.py:372-408; reached by predict(augment=True)).
 * ey_scale_img = `scale_img(x.flip(3) if flip_lr else x, ratio, gs)` (utils/torch_utils.py:423-432): bilinear resize
 * (align_corners=False, ATen source-index rule) of the planar NCHW image x [B,C,H,W] to hs x ws = int(H*r) x int(W*r), written into the
 * top-left corner of y [B,C,Hp,Wp] (Hp,Wp = ceil(H*r/gs)*gs, ...), the rest filled with pad_value (0.447).  x and y must not alias.
 * ey_tta_merge = `_descale_pred` (:388-397) + the anchor slice `_clip_augmented` (:399-408) keeps + this scale's columns of
 * `torch.cat(y, -1)`: out[b, r, out_off + a - lo] = f(pred[b, r, a]) for a in [lo, hi), rows 0-3 divided by `scale`, row 0 mirrored
 * (img_w - x) when flip == 3, row 1 (img_h - y) when flip == 2; flip in {0, 2, 3}.  pred [B,no,A] and out [B,no,A_out] fp32. */
int ey_scale_img(int dtype, int B, int C, int H, int W, const void* x, int hs, int ws, int Hp, int Wp, int flip_lr, float pad_value, void* y,
                 ey_stream_t stream);
int ey_tta_merge(int B, int no, int A, const float* pred, int lo, int hi, float scale, int flip, int img_h, int img_w, float* out, long A_out, int out_off,
                 ey_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

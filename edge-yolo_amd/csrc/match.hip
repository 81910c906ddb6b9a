// Validation matching on the device: ey_match_batch gives the true positives of a batch's kept rows at up to 16 IoU thresholds and adds the
// batch to a confusion matrix, one workgroup per image, in one launch.  The algorithm text is match_core.inc.h, shared with the host program
// of the tests; this file gives it the workgroup's lanes (256 threads), carves its scratch out of the LDS and launches it.  DESIGN.md 7t.
#include "common.h"
#define MTC_HD __device__ __host__
#include "match_core.inc.h"

#define MTC_THREADS 256
#define MTC_MAXB 128
#define MTC_LDS_LIMIT (160 * 1024)

namespace {

struct DevLanes {
  __device__ int id() const { return (int)threadIdx.x; }
  __device__ int count() const { return (int)blockDim.x; }
  __device__ void barrier() { __syncthreads(); }
  __device__ void amin(int* p, int v) { atomicMin(p, v); }
  __device__ void amax(mtc::u64* p, mtc::u64 v) { atomicMax(p, v); }
  __device__ void gadd(int* p) { atomicAdd(p, 1); }
};

struct MatchTab {
  int gt_off[MTC_MAXB + 1];
  long iou_off[MTC_MAXB];
  int iou_ld[MTC_MAXB];
  float iouv[mtc::MAX_T];
};

__global__ __launch_bounds__(MTC_THREADS) void match_batch_kernel(MatchTab tab, int max_det, int stride, int Dcap, int Gcap, const float* __restrict__ rows,
                                                                   const int* __restrict__ count, const float* __restrict__ xform,
                                                                   const float* __restrict__ gt, const int* __restrict__ gt_cls,
                                                                   const float* __restrict__ iou, int T, int nc, float cm_conf, float cm_iou,
                                                                   unsigned char* tp, int* matrix) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ float thr[mtc::MAX_T];
  const int b = blockIdx.x;
  if (threadIdx.x < mtc::MAX_T) thr[threadIdx.x] = tab.iouv[threadIdx.x];
  int D = count[b];
  D = D < 0 ? 0 : (D > Dcap ? Dcap : D);  // never past the rows the caller allocated (Dcap = max_det)
  if (iou && D > tab.iou_ld[b]) D = tab.iou_ld[b];  // nor past the columns of the image's matrix
  const int g0 = tab.gt_off[b];
  const int G = tab.gt_off[b + 1] - g0;  // 0 <= G <= Gcap: checked on the host
  mtc::Job J;
  J.D = D; J.G = G; J.T = T; J.nc = nc; J.stride = stride;
  J.rows = rows + (size_t)b * max_det * stride;
  J.xform = xform ? xform + 5 * (size_t)b : nullptr;
  J.gbox = iou ? nullptr : gt + 4 * (size_t)g0;
  J.gcls = gt_cls + g0;
  J.iou = iou ? iou + tab.iou_off[b] : nullptr;
  J.ld = iou ? tab.iou_ld[b] : 0;
  J.iouv = thr;
  J.cm_conf = cm_conf; J.cm_iou = cm_iou;
  J.tp = tp ? tp + (size_t)b * max_det * T : nullptr;
  J.matrix = matrix;
  // the scratch, sized for (Dcap, Gcap) by mtc::scratch_bytes: the 8-byte keys first
  unsigned char* p = lds;
  J.cmkey = nullptr; J.cg = nullptr; J.lbox = nullptr; J.taker = nullptr; J.dg = nullptr; J.db = nullptr;
  if (matrix) { J.cmkey = (mtc::u64*)p; p += (size_t)Gcap * 8; }
  J.lcls = (int*)p; p += (size_t)Gcap * 4;
  if (matrix) { J.cg = (int*)p; p += (size_t)Dcap * 4; }
  if (!iou) { J.lbox = (float*)p; p += (size_t)Gcap * 16; }
  if (tp) {
    J.taker = (int*)p; p += (size_t)Gcap * T * 4;
    J.dg = (int*)p; p += (size_t)Dcap * 4;
    J.db = (float*)p; p += (size_t)Dcap * 4;
  }
  __syncthreads();  // thr[]
  DevLanes ln;
  mtc::match(ln, J);
}

}  // namespace

extern "C" int ey_match_batch(int B, int max_det, int stride, const float* rows, const int* count, const float* xform, const float* gt, const int* gt_cls,
                              const int* gt_off, const float* iou, const long* iou_off, const int* iou_ld, int T, const float* iouv, int nc, float cm_conf, float cm_iou,
                              uint8_t* tp, int* matrix, ey_stream_t stream) {
  EY_CHECK(B >= 0 && max_det >= 1 && stride >= 6, "ey_match_batch: bad sizes B=%d max_det=%d stride=%d (rows are x1,y1,x2,y2,conf,cls,...)", B, max_det, stride);
  EY_CHECK(T >= 1 && T <= mtc::MAX_T, "ey_match_batch: T=%d thresholds (1..%d are built)", T, (int)mtc::MAX_T);
  EY_CHECK(nc >= 1 && nc <= 46339, "ey_match_batch: nc=%d", nc);
  if (B > MTC_MAXB) return ey_set_error(EY_EUNSUPPORTED, "ey_match_batch: B=%d (up to %d images are built)", B, MTC_MAXB);
  if (B == 0 || (!tp && !matrix)) return EY_OK;
  EY_CHECK(rows && count && gt_off && iouv, "ey_match_batch: null pointer");
  EY_CHECK(gt_off[0] == 0, "ey_match_batch: gt_off[0]=%d must be 0", gt_off[0]);
  MatchTab tab;
  int Gcap = 0;
  for (int b = 0; b < MTC_MAXB; ++b) {
    const bool on = b < B;
    const long g = on ? (long)gt_off[b + 1] - gt_off[b] : 0;
    EY_CHECK(g >= 0, "ey_match_batch: gt_off decreases at image %d", b);
    EY_CHECK(!(on && iou && g) || (iou_off && iou_ld && iou_off[b] >= 0 && iou_ld[b] >= 0), "ey_match_batch: matrix mode needs iou_off[%d], iou_ld[%d] >= 0", b, b);
    if (g > Gcap) Gcap = (int)g;
    tab.gt_off[b + 1] = on ? gt_off[b + 1] : gt_off[B];
    tab.iou_off[b] = (on && iou && g) ? iou_off[b] : 0;
    tab.iou_ld[b] = (on && iou && g) ? iou_ld[b] : max_det;  // (an image without labels has no matrix: nothing of it is read)
  }
  tab.gt_off[0] = 0;
  for (int t = 0; t < mtc::MAX_T; ++t) tab.iouv[t] = t < T ? iouv[t] : 0.f;
  EY_CHECK(gt_off[B] == 0 || (gt_cls && (iou || gt)), "ey_match_batch: null label pointer");
  const size_t lds = mtc::scratch_bytes(max_det, Gcap, T, !iou, tp != nullptr, matrix != nullptr);
  if (lds + sizeof(float) * mtc::MAX_T > MTC_LDS_LIMIT)  // (+ the kernel's static thr[])
    return ey_set_error(EY_EUNSUPPORTED,
                        "ey_match_batch: max_det=%d rows x %d labels of one image x %d thresholds need %zu bytes of LDS, the limit is %d (1024 x 1024 x 16 fits)",
                        max_det, Gcap, T, lds + sizeof(float) * mtc::MAX_T, MTC_LDS_LIMIT);
  if (!ey_lds_reserve<match_batch_kernel>(lds)) return ey_set_error(EY_EUNSUPPORTED, "ey_match_batch: %zu bytes of LDS were refused", lds);
  match_batch_kernel<<<B, MTC_THREADS, lds, (hipStream_t)stream>>>(tab, max_det, stride, max_det, Gcap, rows, count, xform, gt, gt_cls, iou, T, nc, cm_conf,
                                                                    cm_iou, tp, matrix);
  EY_LAUNCH_CHECK("match_batch_kernel");
  return EY_OK;
}

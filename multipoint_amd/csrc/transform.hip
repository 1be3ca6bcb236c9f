// Batched RANSAC similarity and affine estimation for the matched keypoints of P pairs (mp_find_transform,
// mp_refine_transform): what the reference's manual alignment gets from cv2.estimateRigidTransform(ir, opt, False)
// (create_dataset/helper_functions/align.py, the 4-parameter form its optimiser keeps), and the 6-parameter affine model next
// to it.  Not OpenCV's estimateAffinePartial2D / estimateAffine2D bit for bit (absent third-party code with its own RNG and
// an adaptive iteration bound); the route is homography.hip's with another model:
//   T hypotheses per pair, each from S = 2 / 3 distinct random matches (counter-based RNG -> reproducible), exact minimal solve
//   in fp64, score = number of matches with forward error <= threshold, best = most inliers (lowest hypothesis index on ties),
//   final model = least squares over the best consensus set.
// One thread per hypothesis (the matches of the pair sit in LDS); the winner is picked with a 64-bit atomicMax (ransac_kernel,
// mp_ransac.h).  The refit and the refinement are the kernel templates of mp_transform.h, which transform_pooled.hip runs on a
// group's rows in global memory.  As in homography.hip a translation unit instantiates everything for ONE keypoint type,
// MP_TRANSFORM_KP: int here, float in transform_f.hip, which includes this file -- so that whole-number float lists give the
// bits of the int entries.
#include "../../include/multipoint_hip.h"
#include "mp_common.h"
#include "mp_device.h"
#include "mp_transform.h"

#ifndef MP_TRANSFORM_KP
#define MP_TRANSFORM_KP int
#endif

namespace {

template <class Model, class KP>
void find(const KP* kp_yx, const int* kp_count, const int* match_idx, int P, int K, int T, double thr, unsigned long long seed,
          unsigned long long* best, double* H_out, unsigned char* mask, int* n_inliers, hipStream_t s)
{
    const size_t lds1 = (size_t)K * 4 * sizeof(float), lds2 = lds1 + (size_t)K * sizeof(int);
    hipLaunchKernelGGL((ransac_kernel<Model, KP>), dim3((T + 255) / 256, P), dim3(256), lds1, s, kp_yx, kp_count, match_idx,
                       K, T, thr, seed, best);
    hipLaunchKernelGGL((transform_refit_kernel<Model, PairSource<KP>>), dim3(P), dim3(256), lds2, s,
                       PairSource<KP>{kp_yx, kp_count, match_idx, K, mask}, thr, seed, best, H_out, n_inliers);
}

template <class Model, class KP>
void refine(const KP* kp_yx, const int* kp_count, const int* match_idx, int P, int K, double thr, int rounds, double* H_io,
            unsigned char* mask, int* n_inliers, double* cost, hipStream_t s)
{
    const size_t lds = (size_t)K * 4 * sizeof(float) + (size_t)K * sizeof(int);
    hipLaunchKernelGGL((transform_refine_kernel<Model, PairSource<KP>>), dim3(P), dim3(256), lds, s,
                       PairSource<KP>{kp_yx, kp_count, match_idx, K, mask}, thr, rounds, H_io, n_inliers, cost);
}

}  // namespace

template <class KP>
void launch_find_transform(int model, const KP* kp_yx, const int* kp_count, const int* match_idx, int P, int K, int T, double thr,
                           unsigned long long seed, unsigned long long* best, double* H_out, unsigned char* mask, int* n_inliers,
                           hipStream_t s)
{
    if (model == MP_MODEL_SIMILARITY) find<Similarity>(kp_yx, kp_count, match_idx, P, K, T, thr, seed, best, H_out, mask, n_inliers, s);
    else find<Affine>(kp_yx, kp_count, match_idx, P, K, T, thr, seed, best, H_out, mask, n_inliers, s);
}

template void launch_find_transform<MP_TRANSFORM_KP>(int, const MP_TRANSFORM_KP*, const int*, const int*, int, int, int, double,
                                                     unsigned long long, unsigned long long*, double*, unsigned char*, int*,
                                                     hipStream_t);

template <class KP>
void launch_refine_transform(int model, const KP* kp_yx, const int* kp_count, const int* match_idx, int P, int K, double thr,
                             int rounds, double* H_io, unsigned char* mask, int* n_inliers, double* cost, hipStream_t s)
{
    if (model == MP_MODEL_SIMILARITY) refine<Similarity>(kp_yx, kp_count, match_idx, P, K, thr, rounds, H_io, mask, n_inliers, cost, s);
    else refine<Affine>(kp_yx, kp_count, match_idx, P, K, thr, rounds, H_io, mask, n_inliers, cost, s);
}

template void launch_refine_transform<MP_TRANSFORM_KP>(int, const MP_TRANSFORM_KP*, const int*, const int*, int, int, double, int,
                                                       double*, unsigned char*, int*, double*, hipStream_t);

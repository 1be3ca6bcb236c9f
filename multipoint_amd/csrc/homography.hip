// Batched RANSAC homography estimation for the matched keypoints of P pairs: the step that follows
// matching in the reference (predict_align_image_pair.py:205-216, evaluation.py:330-349:
// cv2.findHomography(optical_pts, thermal_pts, cv2.RANSAC, ransacReprojThreshold)).
// OpenCV is a third-party dependency that is absent here and its RANSAC draws from its own RNG, so this is not a
// bit-level restatement ("parity unpinned"); it follows the published algorithm:
//   T hypotheses per pair, each from 4 distinct random matches (counter-based RNG -> reproducible), exact 4-point
//   solve (8x8 Gaussian elimination, fp64), score = number of matches with forward reprojection error <= threshold,
//   best = most inliers (lowest hypothesis index on ties), final model = normalised DLT over the best inlier set.
// One thread per hypothesis (the matches of the pair sit in LDS); the winner is picked with a 64-bit atomicMax.
// OpenCV's last step, the Levenberg-Marquardt polish of the refitted model, is a launch of its own (refine_kernel).
// A pair's matches are located by gather (ordered compaction into LDS) and handed out as a PairView by PairSource; these and the
// scoring kernel are the templates of mp_ransac.h, the refit and the polish those of mp_homography.h, which homography_pooled.hip
// runs on a group's rows in global memory.
// The kernels and launchers are templates on the keypoint type KP -- int pixels, or float sub-pixel positions
// (mp_refine_keypoints) -- which only decides what gather reads.  A translation unit instantiates them for ONE type,
// MP_HOMOGRAPHY_KP: int here, float in homography_f.hip, which includes this file.  Two instantiations side by side change what
// the compiler inlines (a helper with a single caller is inlined, with two it stays a call) and with that the fp64 contractions
// of the refit: the int entries' bits, and their equality with the pooled route's, must not depend on the float entries.
#include "mp_common.h"
#include "mp_device.h"
#include "mp_homography.h"

#ifndef MP_HOMOGRAPHY_KP
#define MP_HOMOGRAPHY_KP int
#endif

template <class KP>
void launch_ransac_homography(const KP* kp_yx, const int* kp_count, const int* match_idx, int P, int K, int T, double thr,
                              unsigned long long seed, unsigned long long* best, double* H_out, unsigned char* mask,
                              int* n_inliers, hipStream_t s)
{
    const size_t lds1 = (size_t)K * 4 * sizeof(float), lds2 = lds1 + (size_t)K * sizeof(int);
    hipLaunchKernelGGL((ransac_kernel<Homography, KP>), dim3((T + 255) / 256, P), dim3(256), lds1, s, kp_yx, kp_count, match_idx, K, T, thr, seed, best);
    hipLaunchKernelGGL(refit_kernel<PairSource<KP>>, dim3(P), dim3(256), lds2, s, PairSource<KP>{kp_yx, kp_count, match_idx, K, mask}, thr,
                       seed, best, H_out, n_inliers);
}

template void launch_ransac_homography<MP_HOMOGRAPHY_KP>(const MP_HOMOGRAPHY_KP*, const int*, const int*, int, int, int, double,
                                                         unsigned long long, unsigned long long*, double*, unsigned char*, int*,
                                                         hipStream_t);

// mask must be zeroed by the caller (only the matched optical keypoints are written)
template <class KP>
void launch_refine_homography(const KP* kp_yx, const int* kp_count, const int* match_idx, int P, int K, double thr, int iters,
                              double* H_io, unsigned char* mask, int* n_inliers, double* cost, hipStream_t s)
{
    const size_t lds = (size_t)K * 4 * sizeof(float) + (size_t)K * sizeof(int);
    hipLaunchKernelGGL(refine_kernel<PairSource<KP>>, dim3(P), dim3(256), lds, s, PairSource<KP>{kp_yx, kp_count, match_idx, K, mask}, thr,
                       iters, H_io, n_inliers, cost);
}

template void launch_refine_homography<MP_HOMOGRAPHY_KP>(const MP_HOMOGRAPHY_KP*, const int*, const int*, int, int, double, int,
                                                         double*, unsigned char*, int*, double*, hipStream_t);

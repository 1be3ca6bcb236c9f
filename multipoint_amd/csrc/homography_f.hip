// The per-pair homography estimators on float keypoints (mp_find_homography_f, mp_refine_homography_f): homography.hip compiled
// for KP = float.  A translation unit of its own, so that each holds one instantiation (homography.hip says why).
#define MP_HOMOGRAPHY_KP float
#include "homography.hip"

// The per-pair similarity / affine estimators on float keypoints (mp_find_transform_f, mp_refine_transform_f): transform.hip
// compiled for KP = float.  A translation unit of its own, so that each holds the same instantiations for one keypoint type.
#define MP_TRANSFORM_KP float
#include "transform.hip"

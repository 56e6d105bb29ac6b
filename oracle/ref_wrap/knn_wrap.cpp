// C entry point of the reference's SimpleKNN::knn for tests/reference_builds.py (compiled and linked with the copied,
// unedited simple_knn.cu by oracle/reference_build.py; nothing of the reference is in this file).
#include "cuda_runtime.h"
#include "simple_knn.h"

extern "C" int bsr_ref_knn(int P, const float* points, float* mean_dists) {
    SimpleKNN::knn(P, (float3*)points, mean_dists);
    return (int)hipDeviceSynchronize();
}

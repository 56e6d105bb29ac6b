"""``simple_knn._C`` on the MI355X: ``distCUDA2`` (``submodules/simple-knn/ext.cpp:15-17``, ``spatial.cu``) with the
extension's signature, backed by ``bloomscene_amd.knn.mean_dist3``.

``distCUDA2(points)``: float32 ``[P, 3]`` on the GPU -> float32 ``[P]``, the mean of the three smallest squared distances
from each point to the others (``include/bloomscene_knn.h`` states the function bit for bit).  A wrong dtype raises
TypeError, a wrong shape or a CPU tensor ValueError (there is no CPU path).
"""
from bloomscene_amd.knn import mean_dist3 as _mean_dist3


def distCUDA2(points):
    return _mean_dist3(points)

"""Import shim: BloomScene's ``scene/gaussian_model.py:20`` does ``from simple_knn._C import distCUDA2`` (the CUDA
extension of ``submodules/simple-knn``).  With this repository on ``sys.path`` that import resolves here, to the
MI355X-native search of ``bloomscene_amd.knn`` (C ABI ``include/bloomscene_knn.h``).  Importing needs no GPU.
"""

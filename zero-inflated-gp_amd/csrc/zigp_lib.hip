// Single translation unit of libzigp.so: the dense and Kronecker paths share the GEMM core and kernels of
// zigp_kernels.h (plain __global__ definitions), so they are compiled together.
#include "zigp_dense.hip"
#include "zigp_kron.hip"
#include "zigp_density.hip"
#include "zigp_score.hip"
#include "zigp_paths.hip"
#include "zigp_kronpaths.hip"
#include "zigp_ensemble.hip"
#include "zigp_kmeans.hip"
#include "zigp_comm.hip"

// Shard forms (SH = true) of the matrix-free KKT diagonal kernels (ctd_diag_kernels.hpp: hdiag, jsq_rows, jsq_cols) of one registry
// entry (EstimateInitialConditionOCP): a translation unit of their own, so that they compile beside the whole-grid forms.
#include "ctd_diag_kernels.hpp"
namespace ctd {
CTD_INSTANTIATE_DIAG_SHARD(EstimateInitialConditionOCP)
}

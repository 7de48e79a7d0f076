// Matrix-free KKT diagonal kernels (ctd_diag_kernels.hpp: hdiag, jsq_rows, jsq_cols) of one registry entry (EstimateRotationRateOCP).
#include "ctd_diag_kernels.hpp"
namespace ctd {
CTD_INSTANTIATE_DIAG(EstimateRotationRateOCP)
}

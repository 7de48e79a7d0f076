// Matrix-free KKT diagonal kernels (ctd_diag_kernels.hpp: hdiag, jsq_rows, jsq_cols) of one registry entry (DoubleIntegratorFreeT0TfOCP).
#include "ctd_diag_kernels.hpp"
namespace ctd {
CTD_INSTANTIATE_DIAG(DoubleIntegratorFreeT0TfOCP)
}

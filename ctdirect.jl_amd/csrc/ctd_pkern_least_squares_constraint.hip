// Matrix-free Jacobian product kernels (ctd_prod_kernels.hpp) of one registry entry (LeastSquaresConstraintOCP).
#include "ctd_prod_kernels.hpp"
namespace ctd {
CTD_INSTANTIATE_PROD(LeastSquaresConstraintOCP)
}

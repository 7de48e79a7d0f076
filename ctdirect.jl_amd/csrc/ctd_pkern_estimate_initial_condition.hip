// Matrix-free Jacobian and Hessian product kernels (ctd_prod_kernels.hpp, ctd_hprod_kernels.hpp) of one registry entry (EstimateInitialConditionOCP).
#include "ctd_hprod_kernels.hpp"
namespace ctd {
CTD_INSTANTIATE_PROD(EstimateInitialConditionOCP)
CTD_INSTANTIATE_HPROD(EstimateInitialConditionOCP)
}

// Matrix-free Jacobian and Hessian product kernels (ctd_prod_kernels.hpp, ctd_hprod_kernels.hpp, ctd_kkt_kernels.hpp) of one registry entry (EstimateRotationRateOCP).
#include "ctd_kkt_kernels.hpp"
namespace ctd {
CTD_INSTANTIATE_PROD(EstimateRotationRateOCP)
CTD_INSTANTIATE_HPROD(EstimateRotationRateOCP)
CTD_INSTANTIATE_KKT(EstimateRotationRateOCP)
}

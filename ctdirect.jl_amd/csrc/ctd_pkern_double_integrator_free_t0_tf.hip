// Matrix-free Jacobian and Hessian product kernels (ctd_prod_kernels.hpp, ctd_hprod_kernels.hpp, ctd_kkt_kernels.hpp) of one registry entry (DoubleIntegratorFreeT0TfOCP).
#include "ctd_kkt_kernels.hpp"
namespace ctd {
CTD_INSTANTIATE_PROD(DoubleIntegratorFreeT0TfOCP)
CTD_INSTANTIATE_HPROD(DoubleIntegratorFreeT0TfOCP)
CTD_INSTANTIATE_KKT(DoubleIntegratorFreeT0TfOCP)
}

// Matrix-free Jacobian and Hessian product kernels (ctd_prod_kernels.hpp, ctd_hprod_kernels.hpp, ctd_kkt_kernels.hpp) of one registry entry (DoubleIntegratorPathOCP).
#include "ctd_kkt_kernels.hpp"
namespace ctd {
CTD_INSTANTIATE_PROD(DoubleIntegratorPathOCP)
CTD_INSTANTIATE_HPROD(DoubleIntegratorPathOCP)
CTD_INSTANTIATE_KKT(DoubleIntegratorPathOCP)
}

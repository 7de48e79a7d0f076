// Matrix-free Jacobian and Hessian product kernels (ctd_prod_kernels.hpp, ctd_hprod_kernels.hpp, ctd_kkt_kernels.hpp) of one registry entry (StagewiseScalarOCP).
#include "ctd_kkt_kernels.hpp"
namespace ctd {
CTD_INSTANTIATE_PROD(StagewiseScalarOCP)
CTD_INSTANTIATE_HPROD(StagewiseScalarOCP)
CTD_INSTANTIATE_KKT(StagewiseScalarOCP)
}

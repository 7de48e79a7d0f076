// Matrix-free Jacobian and Hessian product kernels (ctd_prod_kernels.hpp, ctd_hprod_kernels.hpp, ctd_kkt_kernels.hpp) of one registry entry (QuadrotorOCP).
#include "ctd_kkt_kernels.hpp"
namespace ctd {
CTD_INSTANTIATE_PROD(QuadrotorOCP)
CTD_INSTANTIATE_HPROD(QuadrotorOCP)
CTD_INSTANTIATE_KKT(QuadrotorOCP)
}

// Matrix-free Jacobian and Hessian product kernels (ctd_prod_kernels.hpp, ctd_hprod_kernels.hpp, ctd_kkt_kernels.hpp) of one registry entry (Quadrotor12OCP).
#include "ctd_kkt_kernels.hpp"
namespace ctd {
CTD_INSTANTIATE_PROD(Quadrotor12OCP)
CTD_INSTANTIATE_HPROD(Quadrotor12OCP)
CTD_INSTANTIATE_KKT(Quadrotor12OCP)
}

// Matrix-free Jacobian and Hessian product kernels (ctd_prod_kernels.hpp, ctd_hprod_kernels.hpp, ctd_kkt_kernels.hpp) of one registry entry (GoddardAllOCP).
#include "ctd_kkt_kernels.hpp"
namespace ctd {
CTD_INSTANTIATE_PROD(GoddardAllOCP)
CTD_INSTANTIATE_HPROD(GoddardAllOCP)
CTD_INSTANTIATE_KKT(GoddardAllOCP)
}

// Matrix-free Jacobian product kernels (ctd_prod_kernels.hpp) of one registry entry (Quadrotor12OCP).
#include "ctd_prod_kernels.hpp"
namespace ctd {
CTD_INSTANTIATE_PROD(Quadrotor12OCP)
}

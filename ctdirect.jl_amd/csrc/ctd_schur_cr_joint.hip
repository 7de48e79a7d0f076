// ctd_schur_cr_joint.hip -- the translation unit of the joined form of the log-depth Schur preconditioner (ctd_kkt_schur_cr_joint_*):
// the kernels of ctd_schur_cr.hip instantiated for the argument structs SchurCrJoint*Params, and the family's own kernels and
// launchers, which that file holds under CTD_SCHUR_CR_JOINT beside the device functions they share.  Specification and the order
// of every sum: ctd_schur_cr_joint_kernels.hpp.  Strict rounding, like ctd_schur_cr.hip.
#define CTD_SCHUR_CR_JOINT 1
#include "ctd_schur_cr.hip"

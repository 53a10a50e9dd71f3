// pt_nee_interior.hip -- the interior instances of k_nee (k_nee_interior, k_nee_env_interior, k_nee_tiles_interior, k_nee_env_tiles_interior;
// pt_set_material_interior) and their launcher, launch_nee_interior: pt_nee.hip's one body, nee_frame, instantiated with
// INTERIOR in a translation unit of its own, as pt_nee_medium.hip and pt_nee_grid.hip are, so that the other ten families' instances compile
// exactly as they did before these existed.
#define PT_NEE_INTERIOR_TU 1
#include "pt_nee.hip"

// pt_nee_lighttree.hip -- the light-tree instances of k_nee (k_nee_lighttree, k_nee_env_lighttree, k_nee_tiles_lighttree, k_nee_env_tiles_lighttree;
// option light_tree), their launcher, launch_nee_lighttree, and k_debug_light_tree: pt_nee.hip's one body, nee_frame,
// instantiated with LTREE in a translation unit of its own, as pt_nee_medium.hip, pt_nee_grid.hip and pt_nee_interior.hip are, so that the other
// eleven families' instances compile exactly as they did before these existed.
#define PT_NEE_LIGHTTREE_TU 1
#include "pt_nee.hip"

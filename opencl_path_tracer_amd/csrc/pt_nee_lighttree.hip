// pt_nee_lighttree.hip -- the light-tree instances of k_nee (k_nee<kNeeLightTree, ...>; option light_tree), their launcher,
// launch_nee_tu<kNeeLightTree>, and k_debug_light_tree: pt_nee.hip's one body, nee_frame, instantiated for the family in a translation unit of its
// own, as pt_nee_medium.hip, pt_nee_grid.hip and pt_nee_interior.hip are, so that the other eleven families' instances compile exactly as they
// did before these existed.
#define PT_NEE_TU PT_NEE_FAMILY_LIGHTTREE
#include "pt_nee.hip"

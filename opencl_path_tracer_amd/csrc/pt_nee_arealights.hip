// pt_nee_arealights.hip -- the area-light instances of k_nee (k_nee<kNeeAreaLights, ...>; pt_set_area_lights), their launcher,
// launch_nee_tu<kNeeAreaLights>, and k_debug_area_light: pt_nee.hip's one body, nee_frame, instantiated for the family in a translation unit of its
// own, as pt_nee_medium.hip, pt_nee_grid.hip, pt_nee_interior.hip and pt_nee_lighttree.hip are, so that the other twelve families' instances compile
// exactly as they did before these existed.
#define PT_NEE_TU PT_NEE_FAMILY_AREALIGHTS
#include "pt_nee.hip"

// pt_nee_interior.hip -- the interior instances of k_nee (k_nee<kNeeInterior, ...>; pt_set_material_interior) and their
// launcher, launch_nee_tu<kNeeInterior>: pt_nee.hip's one body, nee_frame, instantiated for the family in a translation unit of its own, as
// pt_nee_medium.hip and pt_nee_grid.hip are, so that the other families' instances compile exactly as they did before these existed.
#define PT_NEE_TU PT_NEE_FAMILY_INTERIOR
#include "pt_nee.hip"

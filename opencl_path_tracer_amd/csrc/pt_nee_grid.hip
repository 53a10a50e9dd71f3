// pt_nee_grid.hip -- the grid instances of k_nee (k_nee<kNeeGrid, ...>; pt_set_medium_density) and their launcher,
// launch_nee_tu<kNeeGrid>: pt_nee.hip's one body, nee_frame, instantiated for the family in a translation unit of its own, as pt_nee_medium.hip is,
// so that the other families' instances compile exactly as they did before these existed.
#define PT_NEE_TU PT_NEE_FAMILY_GRID
#include "pt_nee.hip"

// pt_nee_grid.hip -- the grid instances of k_nee (k_nee_grid, k_nee_env_grid, k_nee_tiles_grid, k_nee_env_tiles_grid; pt_set_medium_density,
// DESIGN.md section 5.20) and their launcher, launch_nee_grid: pt_nee.hip's one body, nee_frame, instantiated with GRID in a translation unit
// of its own, as pt_nee_medium.hip is, so that the other nine families' instances compile exactly as they did before these existed.
#define PT_NEE_GRID_TU 1
#include "pt_nee.hip"

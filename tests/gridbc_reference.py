"""The compiled grid problems WITH A KIND PER SIDE (csrc/nk_grid.hip, NK_GRID_SIDES): the sources and per-stencil-point formulas
of the four tables grid_reference, grid3_reference, grid_r2_reference and gridf_reference, taken as they are, under other sides
(grid_core.Problem.with_boundary). Where a stencil point lands under each kind, what happens when several land on one node, and
the bound are grid_core's.

A boundary here is a tuple of 2·dim kinds: (x-lo, x-hi, y-lo, y-hi[, z-lo, z-hi])."""
import grid3_reference as G3
import grid_r2_reference as G2
import grid_reference as G1
import gridf_reference as GF
from grid_core import RADIUS, uniform

MN, MF, DI, PE = "mirror_node", "mirror_face", "dirichlet", "periodic"
PROBLEMS = {p.name: p for p in [
    G1.PROBLEMS["bratu"].with_boundary("bratu_mirror_node", uniform(MN, 2)),
    G1.PROBLEMS["bratu"].with_boundary("bratu_mirror_face", uniform(MF, 2)),
    # a channel: periodic along x, a Dirichlet-0 wall below, a symmetry line above
    G1.PROBLEMS["bratu"].with_boundary("bratu_channel", (PE, PE, DI, MN)),
    # a plate free at the low end and held at the high end of both axes: the mirror below, Dirichlet-0 above
    G1.PROBLEMS["bratu"].with_boundary("bratu_plate", (MF, DI, MN, DI)),
    G1.PROBLEMS["brusselator"].with_boundary("brusselator_xface_yper", (MF, MF, PE, PE)),
    # the 9-point box, 2 components and a cross term, mirrored in both axes (a kind of each at every corner): four points merge
    G1.PROBLEMS["box_dirichlet"].with_boundary("box_mirror", (MN, MF, MF, MN)),
    # x mirrored, y Dirichlet-0: at a corner the Dirichlet side wins
    G1.PROBLEMS["box_dirichlet"].with_boundary("box_xnode_ydir", (MN, MN, DI, DI)),
    G2.PROBLEMS["upwind2_dirichlet"].with_boundary("star2_mirror", (MN, MF, MF, MN)),
    G2.PROBLEMS["diamond_dirichlet"].with_boundary("diamond2_mirror", (MF, MN, MN, MF)),
    # the 3-D star, dof 2, three different axes: periodic, Dirichlet-0 below and mirror-node above, mirror-face
    G3.PROBLEMS["brusselator3"].with_boundary("star3_mixed", (PE, PE, DI, MN, MF, MF)),
    G3.PROBLEMS["box3_dirichlet"].with_boundary("box3_mirror", (MN, MF, MF, MF, MF, MN)),
    GF.PROBLEMS["vardiff"].with_boundary("vardiff_mirror_face", uniform(MF, 2)),
]}
# the same sources under the boundary they have in their own tables: what the conservation test and the solves compare with
DIRICHLET_TWIN = {"vardiff_mirror_face": GF.PROBLEMS["vardiff"].with_boundary("vardiff_dirichlet", uniform(DI, 2))}


def sizes(prob):
    """each stencil's existing shapes: the smallest that reach every row wrapping or mirroring (3 × 3, 5 × 5, 3 × 3 × 3), a
    ragged last workgroup and five workgroups (37 × 29), and a long thin grid"""
    if prob.dim == 3:
        return [(3, 3, 3), (7, 6, 5), (37, 29, 3)]
    return [(5, 5), (37, 29)] if RADIUS[prob.stencil] == 2 else [(3, 3), (37, 29), (300, 5)]

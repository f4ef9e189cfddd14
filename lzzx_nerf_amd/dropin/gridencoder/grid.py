"""reference path gridencoder/grid.py -> lzzx_nerf_amd.gridencoder"""
from lzzx_nerf_amd.gridencoder import GridEncoder, TriplaneEncoder, _grid_encode, grid_backward_fixed, grid_encode, set_table_grad, table_grad  # noqa: F401

from .grid import GridEncoder, TriplaneEncoder, grid_encode, set_table_grad, table_grad  # noqa: F401  (reference's __init__ is empty; `from gridencoder import GridEncoder` is what encoding.py does)

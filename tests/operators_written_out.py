"""The sparse products of course5_amd.fit's array-built operators (JacobianOperators, ShapeJacobianOperators) written out,
torch op for torch op: one gather, one multiply and one torch.segment_reduce per product - over the CSR rows for J v, and
for J^T g over the copy sorted by column (a stable argsort).  The tests ask the operators for these bits (torch.equal)."""
import torch


class ByRowAndColumn:
    def __init__(self, row_ptr, col, n_cols: int):
        self.row_ptr, self.col = torch.as_tensor(row_ptr).to(torch.int64), torch.as_tensor(col).to(torch.int64)
        n_rows = self.row_ptr.shape[0] - 1
        row = torch.repeat_interleave(torch.arange(n_rows), self.row_ptr[1:] - self.row_ptr[:-1])
        self.order = torch.argsort(self.col, stable=True)
        self.col_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(self.col, minlength=n_cols), 0)])
        self.row_by_col = row[self.order]

    def to_rows(self, values, v):
        """sum over a row's nonzeros of values * v[col]"""
        return torch.segment_reduce(values * v[self.col], "sum", offsets=self.row_ptr)

    def to_columns(self, values, g):
        """sum over a column's nonzeros of values * g[row] (values in row order: sorted here)"""
        return torch.segment_reduce(values[self.order] * g[self.row_by_col], "sum", offsets=self.col_ptr)


def weighted_image(r, w):
    """W r per pixel as the operators' rhs forms it: the multiply in float32, then float64; ([n_px], [n_px])."""
    g = torch.as_tensor(r).to(torch.float32).reshape(-1, 2)
    if w is not None:
        g = g * torch.as_tensor(w).to(torch.float32).reshape(-1, 2)
    g = g.to(torch.float64)
    return g[:, 0], g[:, 1]


def weights(w, n_px: int):
    """(w_tau, w_I) float64 [n_px] (None: ones)."""
    if w is None:
        return torch.ones(n_px, dtype=torch.float64), torch.ones(n_px, dtype=torch.float64)
    w = torch.as_tensor(w).to(torch.float32).reshape(-1, 2)
    return w[:, 0].to(torch.float64), w[:, 1].to(torch.float64)

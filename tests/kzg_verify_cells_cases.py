"""Helpers of the cell verifier's tests (test_kzg_verify_cells_cases.py, test_kzg_verify_cells_sim.py, test_kzg_verify_cells_abi.py, test_gpu_kzg_verify_cells.py): the
interpolation polynomial of a cell in Python integers (kzg_cells_cases.to_coeffs on the cell's coset), the weighted column sums of the combined check, and whole blobs with their
commitment, cells and proofs from kzg_cases.Setup's test-only tau -- a cell's proof is one multiple of the generator from the oracle.  Nothing here calls the code under test."""
from kzg_cases import R, b32, ZERO48
from kzg_cells_cases import to_coeffs, cells, cell_shift, cell_proof

LANES = 256      # FR_CELL_LANES: the lanes of a workgroup, 256 >> log2_cell cells side by side
WALK = 4         # FR_CELL_WALK: the cells a lane group walks in the sum mode before the launch takes another workgroup


def cells_per_blob(log2_n, log2_cell):
    return 2 << (log2_n - log2_cell)


def interp_coeffs(cell, k, log2_n, log2_cell):
    """a_(k,.): the coefficients of the polynomial of degree < c through the c values of cell k"""
    return to_coeffs(cell, log2_cell, shift=cell_shift(k, log2_n, log2_cell))


def neg_rows(cell_list, idx, log2_n, log2_cell, out=()):
    """what the rows mode writes: -a_(k,i) per cell, all-zero for a cell whose position is in `out`"""
    c = 1 << log2_cell
    return [[0] * c if j in out else [(-a) % R for a in interp_coeffs(v, k, log2_n, log2_cell)] for j, (v, k) in enumerate(zip(cell_list, idx))]


def neg_sums(cell_list, idx, weights, log2_n, log2_cell, out=()):
    """what the sum mode writes: -S_i, S_i = sum_k r_k a_(k,i) over the cells that are not out"""
    c = 1 << log2_cell
    s = [0] * c
    for j, (v, k, w) in enumerate(zip(cell_list, idx, weights)):
        if j not in out:
            for i, a in enumerate(interp_coeffs(v, k, log2_n, log2_cell)):
                s[i] = (s[i] + w * a) % R
    return [(-x) % R for x in s]


def cell_bytes(cell):
    return b''.join(b32(v) for v in cell)


class Blob:
    """a polynomial given by its values, with what a verifier receives: the commitment, the cells, and (on demand, one oracle multiplication each) the cells' proofs"""
    def __init__(self, setup, f, log2_n, log2_cell):
        self.setup, self.f, self.log2_n, self.log2_cell = setup, list(f), log2_n, log2_cell
        self.coef = to_coeffs(self.f, log2_n)
        self.commitment = setup.commit(self.f, log2_n)
        self.cells = cells(self.f, log2_n, log2_cell)
        self._proofs = {}

    def proof(self, k):
        if k not in self._proofs:
            self._proofs[k] = cell_proof(self.setup, self.coef, k, self.log2_n, self.log2_cell)
        return self._proofs[k]

    def cell(self, k):
        return cell_bytes(self.cells[k])


def random_blob(setup, log2_n, log2_cell, rnd, degree=None):
    """degree: None = a random blob; else a polynomial of that degree bound (degree 0: the zero polynomial), given by its values"""
    from kzg_cells_cases import to_evals
    n = 1 << log2_n
    if degree is None:
        return Blob(setup, [rnd.randrange(R) for _ in range(n)], log2_n, log2_cell)
    coef = [rnd.randrange(1, R) for _ in range(degree)] + [0] * (n - degree)
    return Blob(setup, to_evals(coef, log2_n), log2_n, log2_cell)


class Call:
    """the arguments of one nbls_kzg_verify_cells call as lists, built cell by cell"""
    def __init__(self, blobs):
        self.blobs = blobs
        self.commitments = [b.commitment for b in blobs]
        self.ci, self.ki, self.cells, self.proofs = [], [], [], []

    def add(self, blob_no, k):
        b = self.blobs[blob_no]
        self.ci.append(blob_no)
        self.ki.append(k)
        self.cells.append(b.cell(k))
        self.proofs.append(b.proof(k))
        return len(self.ci) - 1

    def add_all(self, rnd=None):
        order = [(i, k) for i, b in enumerate(self.blobs) for k in range(len(b.cells))]
        if rnd is not None:
            rnd.shuffle(order)
        for i, k in order:
            self.add(i, k)
        return self

    def args(self):
        return self.commitments, self.ci, self.ki, self.cells, self.proofs


def with_element(cell, j, value):
    """the cell's bytes with element j replaced"""
    return cell[:32 * j] + b32(value) + cell[32 * j + 32:]


def bumped(cell, j):
    """element j plus one mod r: still canonical, no longer the polynomial's value"""
    return with_element(cell, j, (int.from_bytes(cell[32 * j:32 * j + 32], 'big') + 1) % R)


__all__ = ['ZERO48', 'LANES', 'WALK', 'cells_per_blob', 'interp_coeffs', 'neg_rows', 'neg_sums', 'cell_bytes', 'Blob', 'random_blob', 'Call', 'with_element', 'bumped']

"""The model of xsg_count_literals_csr (include/xsg.h, "counts per chunk and literal"): pure Python, no GPU.

The rows of tests/literal_matrix_model.py turned into CSR: indptr has a word per row and one more, indices holds the
columns of a row's non-zero words in ascending order, data the words themselves."""
import literal_matrix_model as MM


def from_rows(rows):
    """[[word of chunk c, literal j]] -> (indptr, indices, data) as lists"""
    indptr, indices, data = [0], [], []
    for r in rows:
        for j, v in enumerate(r):
            if v:
                indices.append(j)
                data.append(v)
        indptr.append(len(indices))
    return indptr, indices, data


def csr(blocks, literals, icase=False):
    return from_rows(MM.matrix(blocks, literals, icase))


def to_rows(indptr, indices, data, k):
    """the dense rows of a CSR result (k columns)"""
    rows = []
    for c in range(len(indptr) - 1):
        r = [0] * k
        for e in range(indptr[c], indptr[c + 1]):
            r[indices[e]] = data[e]
        rows.append(r)
    return rows


def well_formed(indptr, indices, data, k):
    """what every CSR result holds whatever it counts: row_ptr from 0, non-decreasing, ending at nnz; columns below k and
    strictly ascending within a row; no entry 0"""
    if not indptr or indptr[0] != 0 or indptr[-1] != len(indices) or len(indices) != len(data):
        return False
    for c in range(len(indptr) - 1):
        lo, hi = indptr[c], indptr[c + 1]
        if hi < lo:
            return False
        row = indices[lo:hi]
        if any(b <= a for a, b in zip(row, row[1:])) or any(j >= k for j in row):
            return False
    return all(v > 0 for v in data)

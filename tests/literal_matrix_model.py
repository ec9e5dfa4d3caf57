"""The model of xsg_count_literals_chunks (include/xsg.h, "counts per chunk and literal"): pure Python, no GPU.

matrix[c][j] is what tests/literal_counts_model.py counts for literal j on chunk c alone; chunks_with[j] is the number of
chunks whose row holds a non-zero word for literal j."""
import literal_counts_model as LM


def matrix(blocks, literals, icase=False):
    """-> [[counts of chunk c in listing order] for c in binding order]"""
    return [LM.counts([b], literals, icase) for b in blocks]


def chunks_with(rows, k):
    """-> [number of rows with a non-zero word in column j for j < k] (k: the list's length, for a binding of 0 chunks)"""
    return [sum(1 for r in rows if r[j] > 0) for j in range(k)]

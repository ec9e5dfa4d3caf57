"""What the GPU tests of a literal list share (tests/test_gpu_set.py, tests/test_gpu_set_edges.py): every tag of a list
through every entry point and accessor, the comparison with the expected dict, XSG_MATCHES against tests/set_model.py, and
a tightly packed binding."""
import numpy as np

import packing as P
import set_model
import xsg

IC = xsg.FLAG_IGNORE_CASE


def list_all_modes(g, literals, flags=0, lines=True, matches=True):
    """GpuSearch.all_modes for a literal list: every tag through xsg_count / xsg_search and every accessor"""
    g.ctx.set_literals(xsg.literal_list(literals), flags)
    s = g.shard
    out = {}
    if matches:
        c = s.count(xsg.COUNT_MATCHES | xsg.WITH_NEWLINES)
        out["count_matches"] = int(c[xsg.CTR_MATCHES])
        out["newlines"] = int(c[xsg.CTR_NEWLINES])
        out["bytes"] = int(c[xsg.CTR_BYTES])
        out["match_byte_offsets"] = s.search_u64(xsg.MATCH_BYTE_OFFSETS).tolist()
        assert s.search_u64_view(xsg.MATCH_BYTE_OFFSETS).tolist() == out["match_byte_offsets"]
    if lines:
        out["count_lines"] = int(s.count(xsg.COUNT_LINES)[xsg.CTR_LINES])
        s.count_begin(xsg.COUNT_LINES | xsg.WITH_NEWLINES)  # the split-phase form: done inside _begin, handed out by _end
        c = s.count_end()
        assert int(c[xsg.CTR_LINES]) == out["count_lines"], "xsg_count_begin/_end differs from xsg_count"
        out.setdefault("newlines", int(c[xsg.CTR_NEWLINES]))
        out.setdefault("bytes", int(c[xsg.CTR_BYTES]))
        assert (int(c[xsg.CTR_NEWLINES]), int(c[xsg.CTR_BYTES])) == (out["newlines"], out["bytes"])
        out["line_byte_offsets"] = s.search_u64(xsg.LINE_BYTE_OFFSETS).tolist()
        out["line_indices"] = s.search_u64(xsg.LINE_INDICES).tolist()
        ls, lo = s.search_lines()
        out["lines"], out["lines_offsets"] = ls, lo.tolist()
        vl, vb, vo = s.search_lines_view()
        ends = np.cumsum(vl.astype(np.int64)) if vl.size else np.zeros(0, dtype=np.int64)
        raw = vb.tobytes()
        assert [raw[int(e) - int(n):int(e)] for e, n in zip(ends, vl)] == ls, "xsg_result_lines_view: lines differ"
        assert vo.tolist() == out["lines_offsets"], "xsg_result_lines_view: offsets differ"
    return out


def check(got, want, what, keys=None):
    for k in keys or want:
        assert got[k] == want[k], (what, k)


def check_matches(g, blocks, literals, flags, what, global_offsets=None):
    got, off = g.shard.search_matches()
    strings, offsets, _ = set_model.matches(blocks, literals, bool(flags & IC), global_offsets)
    assert (got, off.tolist()) == (strings, offsets), (what, "matches")


def bind_tight(g, blocks, fill):
    """chunks packed as tightly as include/xsg.h allows, `fill` in the pads and the guards (tests/packing.py)"""
    import torch
    pk = P.pack_tight(blocks, fill)
    t = torch.from_numpy(pk.host).to("cuda:0")
    base = t.data_ptr() + pk.base
    assert base % 16 == 0
    chunks = xsg.make_chunks(pk.offsets, pk.lengths)
    if g.shard is None:
        g.shard = xsg.Shard(g.ctx, base, pk.capacity, chunks)
    else:
        g.shard.rebind(base, pk.capacity, chunks)
    g.keep = t

"""The chain links (the DP's p, the backtrack's chain ids) are 32-bit indices into their anchor
set, so a set holds fewer than 2^31 anchors: hymet_mm_map checks every batch's anchor count
against that cap as soon as it is known.  HYMET_ANCHOR_CAP lowers the cap, so a small mapping
reaches the error: HYMET_E_ARG with a message, nothing launched on the links -- and the next call
on the same context, without the variable, maps as the oracle does.
"""
import ctypes

import numpy as np
import pytest

from tests._data import mutate, rand_seq, revcomp

pytestmark = pytest.mark.gpu

HYMET_E_ARG = -2


def test_anchor_cap_error_then_clean_call(monkeypatch):
    from hymet_amd import mapper
    from hymet_amd._lib import Gpu, HymetError
    from hymet_amd.seqio import DevicePool, from_records
    from oracle import oracle_lib as ol
    gpu = Gpu(0)
    rng = np.random.default_rng(91)
    base = rand_seq(rng, 80_000)
    refs = [base, mutate(rng, base, 0.03)]
    names = ["NC_000001.1", "NC_000002.1"]
    ss = from_records([(n, "", s) for n, s in zip(names, refs)])
    part = mapper.IndexPart(gpu, ss)
    opt = mapper.MapOpt.asm10()
    opt.resolve_mid_occ(part)
    qs = [("fwd", mutate(rng, base[10_000:40_000], 0.01)), ("rev", revcomp(base[50_000:58_000])),
          ("two", base[1_000:4_000] + refs[1][60_000:66_000])]
    qpool = DevicePool(gpu, from_records([(n, "", s) for n, s in qs]), DevicePool.ALPHA_MINIMAP2)

    monkeypatch.setenv("HYMET_ANCHOR_CAP", "100")     # the pair has thousands of anchors
    with pytest.raises(HymetError) as err:
        mapper.map_part(gpu, part, qpool, opt)
    assert f"({HYMET_E_ARG})" in str(err.value)
    assert "anchors" in str(err.value) and "32-bit" in str(err.value)

    monkeypatch.delenv("HYMET_ANCHOR_CAP")
    res = mapper.map_part(gpu, part, qpool, opt)
    oi = ol.MmIndex(refs, names=names)
    oopt = ol.asm10_opt()
    ol._mm_lib().mmo_opt_update_mid_occ(ctypes.byref(oopt), oi.h)
    assert oopt.mid_occ == opt.mid_occ
    for qi, (name, s) in enumerate(qs):
        oregs, orl = ol.mm_map(oi, oopt, s, name)
        gregs = res.query(qi)
        assert len(oregs) > 0 and len(gregs) == len(oregs), name
        assert res.rep_len[qi] == orl, name
        g_lines = mapper.paf_lines(name, len(s), gregs, int(res.rep_len[qi]), names, ss.lengths)
        o_lines = ol.format_paf(name, len(s), oregs, orl, names, ss.lengths)
        assert g_lines == o_lines, name

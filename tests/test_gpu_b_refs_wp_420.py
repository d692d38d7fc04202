"""End to end: a 136x72 4:2:0 B picture of a WP slice with two references per list (tests/b_refs_wp_420_content.py) through steps 1-6 of the
pipeline in include/hmme.h ("multi-reference B pictures: explicit weights and 4:2:0 chroma"), every step on device buffers, every step
against its model on the downloaded inputs, and what it is for: the weighted luma prediction is closer to the current picture than the
unweighted one on the same fields.  Every comparison is bit-exact."""
import numpy as np
import pytest

import b_refs_wp_420_content as content
import predict_bi_refs_model as pbrm
import predict_bi_refs_w_model as pbrw
import predict_chroma_bi_refs_model as pcbr
import select_dirs_refs_model as drm
import select_refs_model as srm
from frame_helpers import bind_hmo, mkplane, oracle_origin_refine_w, oracle_origin_search_w, origin_picture
from test_gpu_bipred_refs_w import per_ctu_w, refs_prediction_w

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


def test_end_to_end_on_faded_bands(oracle_lib, hmo):
    import torch
    from hmme import api, synth
    import bipred_refs_bands as bands
    W, H, n, R = content.W, content.H, content.N, content.R
    m = synth.MARGIN
    dev = torch.device("cuda", 0)
    cur_pic, luma, cur_chroma, chroma = content.content()
    wps = [list(content.WPS[l]) for l in range(2)]
    lq = drm.LAMBDA_Q16
    engine = api.Engine(0, 64)
    engine.set_lambda_q16(lq)
    cur = mkplane(engine, cur_pic, W, H, 8)
    lists = [[mkplane(engine, p, W, H, 8) for p in luma[l]] for l in range(2)]
    cplanes = [[[mkplane(engine, p, W // 2, H // 2, 8) for p in chroma[l][r]] for r in range(R)] for l in range(2)]
    try:
        fp, fp_bi, sel, bits = api.FrameParams(bands.SR_UNI, 1, 8, 0, n), api.FrameParams(bands.SR_BI, 1, 8, 0, n), api.SelectParams(64), bands.bits()
        tab = lambda: (torch.zeros((2, R, n, 593, 2), dtype=torch.int16, device=dev), torch.zeros((2, R, n, 593), dtype=torch.int32, device=dev))
        (d_mv, d_sad), (d_q, d_c), (d_bmv, d_bsad), (d_bq, d_bc) = tab(), tab(), tab(), tab()
        d_uni = torch.zeros((2, n, 64, 2), dtype=torch.int16, device=dev)
        d_uref = torch.zeros((2, n, 64), dtype=torch.uint8, device=dev)
        d_field = torch.full((1, 2, n, 64, 2), 0x5A5A, dtype=torch.int16, device=dev)
        d_ref = torch.full((1, 2, n, 64), 0x6B, dtype=torch.uint8, device=dev)
        d_dir = torch.full((1, n, 64), 0xA7, dtype=torch.uint8, device=dev)
        d_slot = torch.zeros((1, n, 64), dtype=torch.int16, device=dev)
        d_cc = torch.zeros((1, n), dtype=torch.int32, device=dev)
        d_img = torch.full((H, W), 0xEE, dtype=torch.uint8, device=dev)
        d_plain = torch.full((H, W), 0xEE, dtype=torch.uint8, device=dev)
        d_cb, d_cr = (torch.full((H // 2, W // 2), 0xEE, dtype=torch.uint8, device=dev) for _ in range(2))
        d_res = torch.full((H, W), 0x7777, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        for l in range(2):                                                      # 1: the weighted uni pass of each list over its references
            engine.search_pairs_w_device([cur] * R, lists[l], fp, wps[l], None, d_mv[l].data_ptr(), d_sad[l].data_ptr(), 0)
            engine.refine_pairs_w_device([cur] * R, lists[l], fp, wps[l], None, d_mv[l].data_ptr(), 1, d_q[l].data_ptr(), d_c[l].data_ptr(), 0)
        # 2: the reference per PU, the two lists as the call's two "pictures"
        engine.select_refs_device(W, H, 2, R, fp, sel, srm.hm_ref_cost(R, lq), d_q.data_ptr(), d_c.data_ptr(), None, d_uni.data_ptr(), d_uref.data_ptr(), None, None, 0)
        for l in range(2):                                                      # 3: the weighted bi pass of list l against list 1-l's field and indices
            engine.search_frame_bi_refs_w_device(cur, lists[l], lists[1 - l], fp_bi, wps[l], wps[1 - l], d_uni[1 - l].data_ptr(), d_uref[1 - l].data_ptr(), 64, None,
                                                 None, d_bmv[l].data_ptr(), d_bsad[l].data_ptr(), 0)
            engine.refine_frame_bi_refs_w_device(cur, lists[l], lists[1 - l], fp_bi, wps[l], wps[1 - l], d_uni[1 - l].data_ptr(), d_uref[1 - l].data_ptr(), 64, None,
                                                 None, d_bmv[l].data_ptr(), 1, d_bq[l].data_ptr(), d_bc[l].data_ptr(), 0)
        # 4: direction and reference per PU (cost tables only: no weighted form); 5: luma and chroma predictions; 6: the residual
        engine.select_dirs_refs_device(W, H, 1, R, fp, sel, [api.DirRefsParams(bits.dir_bits, bits.n_refs, bits.ref_bits, bits.l1_valid_mask)], d_q.data_ptr(), d_c.data_ptr(),
                                       d_bq.data_ptr(), d_bc.data_ptr(), d_uni.data_ptr(), d_uref.data_ptr(), None, d_field.data_ptr(), d_ref.data_ptr(), d_dir.data_ptr(),
                                       d_slot.data_ptr(), d_cc.data_ptr(), 0)
        engine.predict_bi_refs_w_device(lists[0], lists[1], fp, wps[0], wps[1], d_field.data_ptr(), d_dir.data_ptr(), d_ref.data_ptr(), 64, d_img.data_ptr(), W, 0)
        engine.predict_bi_refs_device(lists[0], lists[1], fp, d_field.data_ptr(), d_dir.data_ptr(), d_ref.data_ptr(), 64, d_plain.data_ptr(), W, 0)
        c0, c1 = content.chroma_flat(cplanes)
        cw0, cw1 = content.chroma_wps_flat()
        engine.predict_chroma_bi_refs_device(c0, c1, W, H, fp, d_field.data_ptr(), d_dir.data_ptr(), d_ref.data_ptr(), 64, d_cb.data_ptr(), d_cr.data_ptr(), W // 2,
                                             weights0=cw0, weights1=cw1)
        engine.residual_pairs_device([cur], [d_img.data_ptr()], W, fp, d_slot.data_ptr(), 64, 1, [d_res.data_ptr()], 2 * W, None, None, None, 0)
        torch.cuda.synchronize()
        host = lambda t: t.cpu().numpy()
        mv_int, mv_uni, cost_uni, mv_bi, cost_bi = host(d_mv), host(d_q), host(d_c).view(np.uint32), host(d_bq), host(d_bc).view(np.uint32)
        uni_field, uni_ref = host(d_uni), host(d_uref)
        # step 1 against the oracle's weighted per-CTU search and refinement: the current picture as the "origin", two CTUs per reference
        cur_org = np.ascontiguousarray(cur_pic[m:, m:])
        for l in range(2):
            for r in range(R):
                smv, ssad = oracle_origin_search_w(oracle_lib, cur_org, luma[l][r], W, H, bands.SR_UNI, None, None, lq, 8, wps[l][r], [1, 4])
                assert np.array_equal(mv_int[l, r][[1, 4]], smv) and np.array_equal(host(d_sad).view(np.uint32)[l, r][[1, 4]], ssad), (l, r)
                sq, sc = oracle_origin_refine_w(oracle_lib, cur_org, luma[l][r], W, H, smv[:1], None, lq, 1, 8, wps[l][r], [1])
                assert np.array_equal(mv_uni[l, r][[1]], sq) and np.array_equal(cost_uni[l, r][[1]], sc), (l, r)
        # steps 2 and 4 against the models on the downloaded tables
        for l in range(2):
            f, r, _, _, _ = srm.select_refs_picture(mv_uni[l], cost_uni[l], sel, W, H, srm.hm_ref_cost(R, lq), 0, None, lq, None)
            assert np.array_equal(uni_field[l], f) and np.array_equal(uni_ref[l], r), l
        mf, mr, md, ms, mc = drm.select_dirs_refs_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, uni_ref, sel, W, H, bits, 0, None, lq)
        assert np.array_equal(host(d_field)[0], mf) and np.array_equal(host(d_ref)[0], mr) and np.array_equal(host(d_dir)[0], md)
        assert np.array_equal(host(d_slot)[0].view(np.uint16), ms) and np.array_equal(host(d_cc)[0].view(np.uint32), mc)
        # step 3: the per-CTU weighted calls on the origin of the downloaded field, both lists, both references, two CTUs
        for l in range(2):
            org = origin_picture(cur_pic, refs_prediction_w(hmo, luma[1 - l], wps[1 - l], W, H, 8, uni_field[1 - l], uni_ref[1 - l]), W, H)
            for r in range(R):
                smv, ssad = per_ctu_w(engine, org, luma[l][r], W, H, 8, bands.SR_BI, None, None, wps[l][r], [1, 4])
                assert np.array_equal(host(d_bmv)[l, r][[1, 4]], smv) and np.array_equal(host(d_bsad).view(np.uint32)[l, r][[1, 4]], ssad), (l, r)
                sq, sc = per_ctu_w(engine, org, luma[l][r], W, H, 8, bands.SR_BI, None, None, wps[l][r], [1, 4], smv)
                assert np.array_equal(mv_bi[l, r][[1, 4]], sq) and np.array_equal(cost_bi[l, r][[1, 4]], sc), (l, r)
        # what it is for, first on the models: the weighted prediction of the device's fields is closer to the current picture
        want = pbrw.pred_picture(hmo, luma[0], luma[1], wps[0], wps[1], W, H, 8, mf, md, mr, np.full((H, W), 0xEE, np.int64))
        want_plain = pbrm.pred_picture(hmo, luma[0], luma[1], W, H, 8, mf, md, mr, np.full((H, W), 0xEE, np.int64))
        assert content.sse(want, cur_pic) < content.sse(want_plain, cur_pic), (content.sse(want, cur_pic), content.sse(want_plain, cur_pic))
        # step 5 against the models, step 6 against the difference
        pred, plain = host(d_img), host(d_plain)
        assert np.array_equal(pred, want) and np.array_equal(plain, want_plain)
        assert content.sse(pred, cur_pic) < content.sse(plain, cur_pic)
        cwant = pcbr.bi_refs_picture(hmo, content.chroma_comps(chroma), W, H, 8, mf, md, mr, tuple(np.full((H // 2, W // 2), 0xEE, np.int64) for _ in range(2)),
                                     [[list(content.CHROMA_WPS[c][l]) for l in range(2)] for c in range(2)])
        assert np.array_equal(host(d_cb), cwant[0]) and np.array_equal(host(d_cr), cwant[1]) and not np.array_equal(cwant[0], cwant[1])
        assert np.array_equal(host(d_res), cur_pic[m:m + H, m:m + W].astype(np.int16) - pred.astype(np.int16))
    finally:
        for p in [cur] + lists[0] + lists[1] + [p for l in cplanes for r in l for p in r]:
            p.close()
        engine.close()

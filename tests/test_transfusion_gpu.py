"""pdm_tf_proposals, pdm_tf_decode, TransFusionHead and the TransFusion detector on the GPU: against the reference fixture
(tests/golden/gen_transfusion_fixtures.py) and against the torch formulations kept next to the operators."""
import numpy as np
import pytest
import torch

import pillarnet_reference as pnr
import sparse_conv_reference as scr
import transfusion_case as tc
from arena import Arena
from pdm_ssd_amd import transfusion_ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


# ---- proposals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag, exempt', [('nus', [8, 9]), ('kitti', [])])
def test_proposals_on_the_fixture(tag, exempt):
    fx = tc.fixture()
    index, cls, qhs, pos = transfusion_ops.proposals(torch.from_numpy(fx[f'{tag}.dense_heatmap']).to(DEV), tc.P, 3, exempt, tc.H)
    assert index.dtype == torch.int64 and cls.dtype == torch.int64
    assert np.array_equal(index.cpu().numpy(), fx[f'{tag}.index']) and np.array_equal(cls.cpu().numpy(), fx[f'{tag}.cls'])
    assert np.array_equal(pos.cpu().numpy(), fx[f'{tag}.query_pos'])
    tc.close(qhs.cpu().numpy(), fx[f'{tag}.query_heatmap_score'], 1e-6)


def separated_logits(B, C, H, W, seed):
    """logits whose sigmoid values are all distinct and at least 1e-4 apart inside a sample: a permutation of a grid"""
    rng = np.random.default_rng(seed)
    n = C * H * W
    s = np.stack([rng.permutation(np.linspace(0.02, 0.98, n)) for _ in range(B)])
    return np.log(s / (1 - s)).astype(np.float32).reshape(B, C, H, W)


def same_proposals(logits, P, k, exempt, y_size):
    got = transfusion_ops.proposals(logits, P, k, exempt, y_size)
    want = transfusion_ops.proposals_torch(logits, P, k, exempt, y_size)
    for g, w in zip(got[:2], want[:2]):
        assert torch.equal(g, w)
    assert torch.equal(got[3], want[3])
    tc.close(got[2].cpu().numpy(), want[2].cpu().numpy(), 1e-6)
    return got


@pytest.mark.parametrize('C, exempt', [(3, [1, 2]), (10, [8, 9]), (10, [])])
@pytest.mark.parametrize('k', [1, 3, 5])
@pytest.mark.parametrize('P', [1, 40])
def test_proposals_against_the_torch_formulation(C, exempt, k, P):
    logits = torch.from_numpy(separated_logits(2, C, 13, 21, 5 + C + k)).to(DEV)
    same_proposals(logits, P, k, exempt, 13)


@pytest.mark.parametrize('P', [1, 40, 900, 4500])
def test_proposals_over_several_slices(P):
    """10 x 31 x 29 = 8990 scores: the local stage cuts them into slices of max(P, 4096): 4096 + 4096 + 798, or 4500 + 4490;
    P = 900 is more than the last slice holds.  Quantised scores tie across slices, so the tie rule has to hold between them."""
    logits = separated_logits(2, 10, 31, 29, 77)
    logits[1] = np.round(logits[1] * 4) / 4                           # sample 1: about 30 distinct values, ties everywhere
    same_proposals(torch.from_numpy(logits).to(DEV), P, 3, [8, 9], 31)


def test_proposals_with_exactly_as_many_survivors_as_queries():
    """five peaks per sample on a ramp that rises with x: every other interior cell has a greater right neighbour and the border
    never survives, so the peaks are ALL the survivors; P = their number takes them all, and query P + 1 scores 0"""
    B, C, H, W = 2, 3, 13, 21
    logits = np.broadcast_to(-6.0 + 0.01 * np.arange(W, dtype=np.float32), (B, C, H, W)).copy()
    peaks = [(0, 2, 3), (1, 6, 10), (2, 10, 18), (0, 5, 5), (1, 11, 2)]
    for b in range(B):
        for j, (c, y, x) in enumerate(peaks):
            logits[b, c, y, x + b] = 1.0 + 0.3 * j
    t = torch.from_numpy(logits).to(DEV)
    index, cls, qhs, _ = same_proposals(t, len(peaks), 3, [], H)
    for b in range(B):
        assert sorted(zip(cls[b].tolist(), index[b].tolist())) == sorted((c, y * W + x + b) for c, y, x in peaks)
    assert float(qhs.max(dim=1).values.min()) > 0.5
    _, cls1, qhs1, _ = same_proposals(t, len(peaks) + 1, 3, [], H)
    assert float(qhs1[:, :, -1].abs().max()) == 0.0 and cls1[:, -1].tolist() == [0, 0]     # a zero score: the lowest flat index


def test_proposals_tie_rule_is_the_lower_flat_index():
    """equal scores in different cells and classes: the reference's argsort leaves their order open; here the lower flat
    (class, y, x) index comes first, as in every ranking operator of this library"""
    B, C, H, W = 1, 3, 13, 21
    logits = np.full((B, C, H, W), -8.0, dtype=np.float32)
    tied = [(2, 7, 7), (0, 9, 4), (1, 3, 15), (0, 3, 15), (2, 2, 2)]
    for c, y, x in tied:
        logits[0, c, y, x] = 2.0
    logits[0, 1, 10, 10] = 3.0
    index, cls, _, _ = same_proposals(torch.from_numpy(logits).to(DEV), 4, 3, [], H)
    flat = sorted(c * H * W + y * W + x for c, y, x in tied)
    want = [1 * H * W + 10 * W + 10] + flat[:3]
    assert (cls[0] * H * W + index[0]).tolist() == want


def test_proposals_in_an_arena():
    fx = tc.fixture()
    arena = Arena(DEV, nbytes=4 << 20)
    logits = arena.put(fx['nus.dense_heatmap'], 4, float('nan'))
    index, cls, qhs, pos = transfusion_ops.proposals(logits, tc.P, 3, [8, 9], tc.H)
    assert np.array_equal(index.cpu().numpy(), fx['nus.index']) and np.array_equal(cls.cpu().numpy(), fx['nus.cls'])
    assert bool(torch.isfinite(qhs).all())
    arena.check()


# ---- decode -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', list(tc.TAGS))
@pytest.mark.parametrize('vel', [True, False])
def test_decode_on_the_fixture(tag, vel):
    tc.check_padded(tag, tc.fixture_decode(tag, transfusion_ops.decode, DEV, vel), vel)


def test_decode_a_sample_without_a_survivor_and_many_queries():
    """P = 700 spans three rounds of the workgroup's scan; sample 1 scores below the threshold everywhere"""
    B, C, P = 2, 4, 700
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(s, generator=g).to(DEV)
    hm, center, height, dim, rot, vel = r(B, C, P), r(B, 2, P) * 5 + 10, r(B, 1, P), r(B, 3, P) * 0.3, r(B, 2, P), r(B, 2, P)
    cls = torch.randint(0, C, (B, P), generator=g).to(DEV)
    qhs = torch.rand((B, C, P), generator=g).to(DEV)
    qhs[1] *= 0.01
    args = (hm, center, height, dim, rot, vel, cls, qhs, 0.05, [0.0, 0.0, -2.0, 8.0, 8.0, 2.0], 0.0, 0.0, 0.05, 0.05, 8)
    got, want = transfusion_ops.decode(*args), transfusion_ops.decode_torch(*args)
    assert got[3].tolist() == want[3].tolist() and got[3][1].item() == 0 and 0 < got[3][0].item() < P
    assert torch.equal(got[2], want[2])
    tc.close(got[0].cpu().numpy(), want[0].cpu().numpy(), 1e-5)
    tc.close(got[1].cpu().numpy(), want[1].cpu().numpy(), 1e-6)


def test_decode_in_an_arena():
    fx, man = tc.fixture(), tc.manifest()
    arena = Arena(DEV, nbytes=4 << 20)
    t = {k: arena.put(fx[f'nus.pred.{k}'], 4 * (1 + i % 3), float('nan')) for i, k in enumerate(tc.MAPS)}
    cls = arena.put(fx['nus.cls'], 8, 0)
    qhs = arena.put(fx['nus.query_heatmap_score'], 12, float('nan'))
    padded = transfusion_ops.decode(t['heatmap'], t['center'], t['height'], t['dim'], t['rot'], t['vel'], cls, qhs, man['score_thresh'],
                                    man['post_center_range'], tc.PC_RANGE[0], tc.PC_RANGE[1], tc.VOXEL[0], tc.VOXEL[1], tc.STRIDE)
    tc.check_padded('nus', padded)
    arena.check()


# ---- the head ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gpu_heads():
    return {tag: tc.build_head(tag, DEV) for tag in tc.TAGS}


@pytest.mark.parametrize('tag', list(tc.TAGS))
def test_head_on_the_device_reproduces_the_fixture(gpu_heads, tag):
    fx, man = tc.fixture(), tc.manifest()
    head = gpu_heads[tag]
    x = torch.from_numpy(fx['spatial_features_2d']).to(DEV)
    seen = {}
    hook = head.decoder.register_forward_hook(lambda m, args, out: seen.update(pos=args[2], out=out))
    with torch.no_grad():
        res = head.predict(x)
    hook.remove()
    assert np.array_equal(head.query_labels.cpu().numpy(), fx[f'{tag}.cls'])            # asserted, not skipped on
    assert np.array_equal(seen['pos'].cpu().numpy(), fx[f'{tag}.query_pos'])
    tc.close(seen['out'].cpu().numpy(), fx[f'{tag}.decoder_out'], man['parity_abs'])
    tc.check_predictions(res, tag, man['parity_abs'])
    out = head({'batch_size': tc.B, 'spatial_features_2d': x})
    assert [len(d['pred_boxes']) for d in out['final_box_dicts']] == man[f'kept.{tag}']
    tc.check_boxes(out['final_box_dicts'], tag, man['parity_abs'])


def test_fused_and_torch_paths_agree(gpu_heads):
    man = tc.manifest()
    x = torch.from_numpy(tc.fixture()['spatial_features_2d']).to(DEV)
    plain = tc.build_head('nus', DEV, use_fused=False)
    with torch.no_grad():
        a, b = gpu_heads['nus'].predict(x), plain.predict(x)
    assert torch.equal(gpu_heads['nus'].query_labels, plain.query_labels)
    for name in tc.MAPS + ('query_heatmap_score',):
        tc.close(a[name].cpu().numpy(), b[name].cpu().numpy(), man['parity_abs'])
    for da, db in zip(gpu_heads['nus'].get_bboxes(a), plain.get_bboxes(b)):
        assert torch.equal(da['pred_labels'], db['pred_labels'])
        tc.close(da['pred_boxes'].cpu().numpy(), db['pred_boxes'].cpu().numpy(), man['parity_abs'])


def test_captured_predict_and_decode_replay_bit_for_bit(gpu_heads):
    head = gpu_heads['nus']
    x = torch.from_numpy(tc.fixture()['spatial_features_2d']).to(DEV)
    with torch.no_grad():
        eager = head.decode_padded(head.predict(x))                 # (the warm-up call as well)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = head.decode_padded(head.predict(x))
    graph.replay()
    torch.cuda.synchronize()
    for e, c in zip(eager, captured):
        assert torch.equal(e, c)


# ---- the detector -----------------------------------------------------------------------------------------------------------------
# chosen on the GPU from seeds 1 .. 12, each with the heat-map head's last layer scaled so that the best logits spread over about
# 2.5 and end near 0: at this seed the torch path's heat-map keeps rank gaps of 2.6e-3 and window gaps of 0.53
DETECTOR_SEED, DETECTOR_HM_GAIN, DETECTOR_HM_BIAS = 2, 54.1, -58.8


def small_detector(seed, hm_gain=None, hm_bias=None):
    """build_transfusion_lidar on a 24 x 24 map (grid 192 x 192 x 40 of 0.1 x 0.1 x 0.2 m voxels), 12 queries.  Every
    parameter is seeded: the head by transfusion_case.fill_transfusion, the two backbones by the fills of the voxel and pillar
    tests (unit-gain weights, set BatchNorm statistics).  With the constructors' initialisation the backbones hand the head
    features of 1e-5 on top of constant shifts: a flat heat-map and nothing but ties."""
    import copy
    from pdm_ssd_amd import detector_config as dc
    cfg = copy.deepcopy(dc.TRANSFUSION_LIDAR_CFG)
    cfg['DENSE_HEAD'].update(NUM_PROPOSALS=12)
    cfg['DENSE_HEAD']['POST_PROCESSING'].update(SCORE_THRESH=0.0, POST_CENTER_RANGE=[-30.0, -30.0, -10.0, 30.0, 30.0, 10.0])
    ds = dc.transfusion_dataset(point_cloud_range=[-9.6, -9.6, -5.0, 9.6, 9.6, 3.0], voxel_size=[0.1, 0.1, 0.2], grid_size=[192, 192, 40])
    torch.manual_seed(seed)
    net = dc.build_transfusion_lidar(cfg, dataset=ds)
    scr.fill_backbone(net.backbone_3d, seed, gain=0.6)
    pnr.fill_pillarnet(net.backbone_2d, seed)
    tc.fill_transfusion(net.dense_head, seed, 1.0, DETECTOR_HM_GAIN if hm_gain is None else hm_gain,
                        DETECTOR_HM_BIAS if hm_bias is None else hm_bias)
    return net.to(DEV).eval()


def synthetic_points(seed, B=2, n=8000):
    """rows (b, x, y, z, intensity, time lag) over the whole range: the points lie near a wavy surface z(x, y) with patches of
    their own, so that the occupied heights, and with them the map's features, change from cell to cell"""
    rng = np.random.default_rng(seed)
    rows = []
    for b in range(B):
        xy = rng.uniform(-9.5, 9.5, (n, 2))
        ph = rng.uniform(0, 6.28, 4)
        z = -1.0 + 1.6 * np.sin(0.9 * xy[:, 0] + ph[0]) * np.cos(0.7 * xy[:, 1] + ph[1]) + 1.2 * np.sin(0.31 * xy[:, 0] * xy[:, 1] + ph[2])
        z = np.clip(z + rng.normal(0, 0.15, n), -4.8, 2.8)
        inten = 0.5 + 0.5 * np.sin(1.3 * xy[:, 0] - 0.8 * xy[:, 1] + ph[3])
        rows.append(np.concatenate([np.full((n, 1), b), xy, z[:, None], inten[:, None], rng.uniform(0, 0.5, (n, 1))], 1))
    return torch.from_numpy(np.concatenate(rows).astype(np.float32)).to(DEV)


def test_detector_eval_forward_and_torch_path_agree():
    net = small_detector(DETECTOR_SEED)
    head = net.dense_head
    pts = synthetic_points(DETECTOR_SEED)
    head.use_fused = False
    with torch.no_grad():
        plain, _ = net({'batch_size': 2, 'points': pts.clone()})
        heat = head.forward_ret_dict['pred_dicts']['dense_heatmap']
    # before the paths are compared: the discrete choices of the torch path's heat-map keep their margins
    margins = tc.proposal_margins(heat.cpu().numpy(), 3, (8, 9), head.num_proposals)
    print('detector heat-map margins', margins)
    tc.check_proposal_margins(margins, head.num_proposals)
    head.use_fused = True
    with torch.no_grad():
        fused, _ = net({'batch_size': 2, 'points': pts.clone()})
    assert len(fused) == 2
    for f, p in zip(fused, plain):
        n = len(f['pred_boxes'])
        assert f['pred_boxes'].shape == (n, 9) and n > 0
        assert int(f['pred_labels'].min()) >= 1 and int(f['pred_labels'].max()) <= 10
        assert float(f['pred_scores'].min()) > 0.0 and float(f['pred_scores'].max()) <= 1.0
        assert torch.equal(f['pred_labels'], p['pred_labels'])
        # two fp32 formulations of one decoder: the fixture's parity_abs (4e-5 at 32 channels, boxes up to 8) times 4 for sums four
        # times as long (128 channels, a 256-wide feed-forward block); a score is a product of two sigmoids, slope <= 1 / 4
        tc.close(f['pred_boxes'].cpu().numpy(), p['pred_boxes'].cpu().numpy(), 1.6e-4)
        tc.close(f['pred_scores'].cpu().numpy(), p['pred_scores'].cpu().numpy(), 4e-5)

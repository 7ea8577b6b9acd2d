#!/usr/bin/env python3
"""Generates tests/golden/ref_transfusion.npz (+ ref_transfusion_manifest.json) by running the REFERENCE's own
TransFusionHead in eval mode on the CPU: pcdet/models/dense_heads/transfusion_head.py with
models/model_utils/transfusion_utils.py and basic_block_2d.py, imported from where they lie, nothing copied, with the
stubs of gen_head_fixtures.install_reference and one more: an empty module as pcdet.ops.iou3d_nms.iou3d_nms_cuda, which
target_assigner/hungarian_assigner.py imports (scipy is present).  Run in the authoring container only; the outputs hold
numbers and key names only.

Shapes (tests/transfusion_case.py): B = 2, H = 12, W = 20 (grid [160, 96, 1] at stride 8; non-square on purpose: it pins
the order of the reference's position table), input_channels 16, HIDDEN_CHANNEL 32, NUM_HEADS 2 (d = 16), FFN_CHANNEL 48,
NUM_PROPOSALS 12, ten nuScenes class names.  Head `nus` has DATASET nuScenes (classes 8 and 9 exempt from the
local-maximum filter), head `kitti` DATASET KITTI (none exempt).

No weights are stored: the generator and the tests fill parameters and BatchNorm statistics from the same seed
(transfusion_case.fill_transfusion); the manifest holds the state-dict keys and shapes and the weights' check sum.

The seed is searched until, on the reference's own numbers, with a margin of 1e-3 each:
  (a) every sample has at least P positive survivors,
  (b) ranks 1 .. P + 1 of the masked scores are pairwise apart,
  (c) every surviving cell among the top P + 1 exceeds each other cell of its window and every non-surviving cell that
      would rank there loses to its window maximum,
  (d) every decoded score and centre is away from its threshold or limit,
  (+) the two heads do not pick the same cells (an exempt class's cell that is no local maximum is among the queries),
  (e) at least one query is dropped by the score threshold, one by a lower and one by an upper limit of the centre range,
      and at least one sample keeps fewer than P.
The score threshold and the centre range are chosen from the reference's unfiltered decode, half way between two
neighbouring values, and written into the manifest.

Parity bound: the reference's head cannot run whole in float64 (its one_hot.float() meets double weights), so the decoder
and the prediction head are run in float32 and in float64 on the same float32 query set, and the float64 boxes are decoded
here in numpy.  With the seeded weights the reference's own float32 run lies up to 5.5e-6 from its float64 run (the decoder's
LayerNorm outputs reach 4, the boxes 8); parity_abs = 4e-5 leaves a second float32 implementation with another summation
order a few times that distance, and the generator fails unless float32 and float64 agree within a quarter of it.
"""
import copy
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_center_head_fixtures import EasyDict  # noqa: E402
from gen_head_fixtures import install_reference  # noqa: E402
import transfusion_case as tc  # noqa: E402

PARITY_ABS = 4e-5
GAIN, HM_GAIN, HM_BIAS = 1.0, 1.5, -3.0


def run_head(ref_tf, dataset, seed, feats, score_thresh=0.0, post_range=(-1e4, -1e4, -1e4, 1e4, 1e4, 1e4)):
    head = ref_tf.TransFusionHead(model_cfg=EasyDict(tc.head_cfg(dataset, score_thresh, post_range)), **tc.head_kwargs())
    total = tc.fill_transfusion(head, seed, GAIN, HM_GAIN, HM_BIAS)
    head.eval()
    seen = {}
    head.decoder.register_forward_hook(lambda m, args, out: seen.update(args=[a.detach().clone() for a in args], out=out.detach().clone()))
    with torch.no_grad():
        res = head.predict(torch.from_numpy(feats))
        res = {k: v.detach().clone() for k, v in res.items()}
        final = head.get_bboxes({k: v.clone() for k, v in res.items()})       # (the reference's decode scales `center` in place)
    return head, total, res, final, seen


def decode64(res64, cls, qhs, stride, voxel, pc_range):
    """float64 numpy restatement of the unfiltered decode -> (boxes (B, P, 9), scores (B, P))"""
    hm = 1.0 / (1.0 + np.exp(-res64['heatmap']))
    at = cls[:, None, :]
    score = (np.take_along_axis(hm, at, 1) * np.take_along_axis(qhs.astype(np.float64), at, 1))[:, 0]
    x = res64['center'][:, 0] * stride * voxel[0] + pc_range[0]
    y = res64['center'][:, 1] * stride * voxel[1] + pc_range[1]
    cols = [x, y, res64['height'][:, 0], *np.exp(res64['dim']).transpose(1, 0, 2), np.arctan2(res64['rot'][:, 0], res64['rot'][:, 1]),
            *res64['vel'].transpose(1, 0, 2)]
    return np.stack(cols, -1), score


def main():
    install_reference()
    sys.modules['pcdet.ops.iou3d_nms.iou3d_nms_cuda'] = types.ModuleType('pcdet.ops.iou3d_nms.iou3d_nms_cuda')
    sys.modules['pcdet.ops.iou3d_nms'].iou3d_nms_cuda = sys.modules['pcdet.ops.iou3d_nms.iou3d_nms_cuda']
    from pcdet.models.dense_heads import transfusion_head as ref_tf
    feats = np.random.default_rng(7).standard_normal((tc.B, tc.CIN, tc.H, tc.W)).astype(np.float32)
    P = tc.P
    for seed in range(300, 1500):
        try:
            runs, margins = {}, {}
            for tag, dataset in tc.TAGS.items():
                runs[tag] = run_head(ref_tf, dataset, seed, feats)
                exempt = (8, 9) if dataset == 'nuScenes' else ()
                margins[tag] = tc.proposal_margins(runs[tag][2]['dense_heatmap'].numpy(), 3, exempt, P)
                tc.check_proposal_margins(margins[tag], P)
            # the exempt classes decide: a query of the nuScenes head is a cell the plain filter drops
            assert not np.array_equal(runs['nus'][4]['args'][2].numpy(), runs['kitti'][4]['args'][2].numpy()), 'the heads pick the same cells'
            # thresholds from the unfiltered decode of the nuScenes head, half way between neighbouring values
            _, _, res, final, _ = runs['nus']
            boxes = np.stack([d['pred_boxes'].numpy() for d in final]).astype(np.float64)
            scores = np.stack([d['pred_scores'].numpy() for d in final]).astype(np.float64)
            assert boxes.shape == (tc.B, P, 9)
            s = np.sort(scores.reshape(-1))
            thresh = float((s[2] + s[3]) / 2)
            xs, ys = np.sort(boxes[..., 0].reshape(-1)), np.sort(boxes[..., 1].reshape(-1))
            zs = np.sort(boxes[..., 2].reshape(-1))
            post = [float((xs[1] + xs[2]) / 2), float(ys[0] - 1.0), float(zs[0] - 1.0), float(xs[-1] + 1.0), float((ys[-3] + ys[-2]) / 2),
                    float(zs[-1] + 1.0)]
            lim = np.array(post)
            for tag in tc.TAGS:
                f = runs[tag][3]
                bx = np.stack([d['pred_boxes'].numpy() for d in f]).astype(np.float64)
                sc = np.stack([d['pred_scores'].numpy() for d in f]).astype(np.float64)
                margins[tag]['decode_gap'] = float(min(np.abs(sc - thresh).min(), np.abs(bx[..., :3] - lim[:3]).min(),
                                                       np.abs(bx[..., :3] - lim[3:]).min()))
                assert margins[tag]['decode_gap'] >= tc.MARGIN, margins[tag]
            low, below, above = scores <= thresh, (boxes[..., :3] < lim[:3]).any(-1), (boxes[..., :3] > lim[3:]).any(-1)
            assert low.any() and below.any() and above.any(), 'a drop reason is missing'
            assert (low & ~below & ~above).any() and (below & ~low).any() and (above & ~low).any(), 'a drop reason never decides alone'
        except AssertionError:
            continue
        break
    else:
        raise SystemExit('no seed meets the conditions')

    out = {'spatial_features_2d': feats}
    manifest = {'seed': seed, 'gain': GAIN, 'hm_gain': HM_GAIN, 'hm_bias': HM_BIAS, 'parity_abs': PARITY_ABS, 'score_thresh': thresh, 'post_center_range': post,
                'margins': margins, 'margin_required': tc.MARGIN}
    gaps = {}
    for tag, dataset in tc.TAGS.items():
        head, total, res, final, seen = run_head(ref_tf, dataset, seed, feats, thresh, post)
        kept = [len(d['pred_boxes']) for d in final]
        assert min(kept) < P, kept
        manifest['weight_sum'] = total
        manifest[f'state.{tag}'] = {k: list(v.shape) for k, v in head.state_dict().items()}
        manifest[f'kept.{tag}'] = kept
        q_feat, flat, q_pos, bev_pos = seen['args']
        out32 = seen['out']                       # (a deep copy of the decoder carries the hook along and would overwrite it)
        out[f'{tag}.dense_heatmap'] = res['dense_heatmap'].numpy()
        out[f'{tag}.cls'] = head.query_labels.numpy().astype(np.int64)
        out[f'{tag}.query_heatmap_score'] = res['query_heatmap_score'].numpy()
        out[f'{tag}.query_pos'] = q_pos.numpy()
        # the cell of a query, from the reference's position table before the flip: bev_pos[n] = (n // y_size + 0.5, n % y_size + 0.5)
        y_size = tc.GRID[1] // tc.STRIDE
        n = np.round((q_pos.numpy()[..., 1] - 0.5) * y_size + (q_pos.numpy()[..., 0] - 0.5)).astype(np.int64)
        assert np.array_equal(res['query_heatmap_score'].numpy(),       # the derived cells are the ones the reference gathered at
                              np.take_along_axis(_masked32(res['dense_heatmap'], tag).reshape(tc.B, 10, -1), n[:, None, :].repeat(10, 1), 2))
        out[f'{tag}.index'] = n
        out[f'{tag}.decoder_out'] = out32.numpy()
        for name in tc.MAPS:
            out[f'{tag}.pred.{name}'] = res[name].numpy()
        for b, d in enumerate(final):
            out[f'{tag}.final.boxes.{b}'] = d['pred_boxes'].numpy()
            out[f'{tag}.final.scores.{b}'] = d['pred_scores'].numpy()
            out[f'{tag}.final.labels.{b}'] = d['pred_labels'].numpy().astype(np.int64)
        # float64 twin of the decoder and the prediction head on the same float32 query set
        dec64, pred64 = copy.deepcopy(head.decoder).double(), copy.deepcopy(head.prediction_head).double()
        with torch.no_grad():
            o64 = dec64(q_feat.double(), flat.double(), q_pos.double(), bev_pos.double())
            r64 = {k: v.numpy() for k, v in pred64(o64).items()}
        r64['center'] = r64['center'] + q_pos.double().permute(0, 2, 1).numpy()
        gap = {'decoder_out': float(np.abs(o64.numpy() - out32.numpy()).max())}
        for name in tc.MAPS:
            gap[name] = float(np.abs(r64[name] - res[name].numpy()).max())
        b64, s64 = decode64(r64, out[f'{tag}.cls'], out[f'{tag}.query_heatmap_score'], tc.STRIDE, tc.VOXEL, tc.PC_RANGE)
        unf = run_head(ref_tf, dataset, seed, feats)[3]
        gap['boxes'] = float(np.abs(b64 - np.stack([d['pred_boxes'].numpy() for d in unf])).max())
        gap['scores'] = float(np.abs(s64 - np.stack([d['pred_scores'].numpy() for d in unf])).max())
        assert max(gap.values()) <= PARITY_ABS / 4, gap
        gaps[tag] = gap
    manifest['float32_to_float64_gap'] = gaps
    np.savez_compressed(os.path.join(HERE, 'ref_transfusion.npz'), **out)
    with open(os.path.join(HERE, 'ref_transfusion_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print('wrote', len(out), 'arrays; seed', seed, 'margins', margins, 'kept', [manifest[f'kept.{t}'] for t in tc.TAGS], 'gaps', gaps)


def _masked32(dense_heatmap, tag):
    """the reference's masked float32 scores, recomputed with its own torch expressions' operators (max_pool2d, ==)"""
    s = dense_heatmap.sigmoid()
    local = torch.zeros_like(s)
    local[:, :, 1:-1, 1:-1] = torch.nn.functional.max_pool2d(s, kernel_size=3, stride=1, padding=0)
    if tag == 'nus':
        local[:, 8:10] = s[:, 8:10]
    return (s * (s == local)).numpy()


if __name__ == '__main__':
    main()

"""SECONDHead from the 2-D map and the rois to the output of its first shared FC block (Conv1d 25088 -> 256, BatchNorm1d, ReLU), three
formulations, at the head's setting (C = 512 on 200 x 176 cells, G = 7) at bs = 32 and bs = 4 with 100 rois a sample: a seeded
smooth map, rois of car size with random headings inside the KITTI range.
  (a) per_sample  the reference's formulation in torch: per sample theta, affine_grid, grid_sample(align_corners=True) of the
                  expanded map, the samples concatenated, then the torch block
  (b) crop        bev_roi_ops.bev_roi_crop (one launch) and the torch block
  (c) fused       bev_roi_ops.bev_roi_crop_fc: the crop and the block without the (R, C G^2) tensor
The forms are called in turn in one process on the same device and inputs, timed with device events around each call after a
warm-up; medians are reported, with the kernel launches of one call as torch.profiler counts them and the peak of bytes allocated
above the inputs during one call; the crop alone is timed as well, with the rate its output is written at.  Results are compared
first.  Prints one JSON line and writes it to profiles/second_iou_rate.json.  No ratio is fixed in advance: the numbers are the
record, and roi_heads/second_head.py's FUSED_FC_DEFAULT follows 'fused_beats_crop_at_every_bs'.

  python tools/second_iou_rate.py [--bs 32 4] [--rois 100] [--calls 7] [--warmup 2] [--no-launch-count] [--out FILE]
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import sparse_conv_rate as scr_tool  # noqa: E402  (timed, launches)
from voxel_rcnn_rate import peak_bytes  # noqa: E402
from pdm_ssd_amd import bev_roi_ops, synthetic  # noqa: E402
from pdm_ssd_amd.config import cfg_from_dict  # noqa: E402
from pdm_ssd_amd.detector_config import SECOND_IOU_CFG, VOXEL_SIZE  # noqa: E402
from pdm_ssd_amd.roi_heads import SECONDHead  # noqa: E402

H, W = 200, 176


def per_sample_pool(rois, feat, pc_range, voxel_size, ratio, G):
    """the reference's roi_grid_pool: one affine_grid and one grid_sample of the expanded map per sample"""
    B, n = rois.shape[0], rois.shape[1]
    C, height, width = feat.shape[1], feat.shape[2], feat.shape[3]
    pooled = []
    for b in range(B):
        r = rois[b]
        x1 = (r[:, 0] - r[:, 3] / 2 - pc_range[0]) / (voxel_size[0] * ratio)
        x2 = (r[:, 0] + r[:, 3] / 2 - pc_range[0]) / (voxel_size[0] * ratio)
        y1 = (r[:, 1] - r[:, 4] / 2 - pc_range[1]) / (voxel_size[1] * ratio)
        y2 = (r[:, 1] + r[:, 4] / 2 - pc_range[1]) / (voxel_size[1] * ratio)
        cosa, sina = torch.cos(r[:, 6]), torch.sin(r[:, 6])
        theta = torch.stack(((x2 - x1) / (width - 1) * cosa, (x2 - x1) / (width - 1) * (-sina), (x1 + x2 - width + 1) / (width - 1),
                             (y2 - y1) / (height - 1) * sina, (y2 - y1) / (height - 1) * cosa, (y1 + y2 - height + 1) / (height - 1)),
                            dim=1).view(-1, 2, 3).float()
        grid = F.affine_grid(theta, torch.Size((n, C, G, G)), align_corners=True)
        pooled.append(F.grid_sample(feat[b].unsqueeze(0).expand(n, C, height, width), grid, align_corners=True))
    return torch.cat(pooled, dim=0)


def smooth_map(bs, C, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    coarse = torch.randn((bs, C, H // 8, W // 8), generator=g, device=dev)
    return (F.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=False) + 0.1 * torch.randn((bs, C, H, W), generator=g, device=dev)).contiguous()


def rounds(fns, calls, warmup):
    """the forms in turn, `warmup + calls` rounds -> the median of each form's timed calls"""
    times = [[] for _ in fns]
    for i in range(warmup + calls):
        for k, fn in enumerate(fns):
            t = scr_tool.timed(fn)[0]
            if i >= warmup:
                times[k].append(t)
    return [statistics.median(t) for t in times]


def run(bs, n_rois, calls, warmup, dev):
    pc_range = list(synthetic.KITTI_RANGE)
    cfg = cfg_from_dict(copy.deepcopy(SECOND_IOU_CFG['ROI_HEAD']))
    torch.manual_seed(0)
    head = SECONDHead(input_channels=512, model_cfg=cfg, num_class=1, point_cloud_range=pc_range, voxel_size=VOXEL_SIZE).to(dev).eval()
    G, C, ratio = head.grid_size, head.in_channel, cfg.ROI_GRID_POOL.DOWNSAMPLE_RATIO
    first = head.shared_fc_layer[0:3]
    cout = first[0].out_channels
    with torch.no_grad():
        first[1].running_var.uniform_(0.5, 1.5)
        first[1].running_mean.uniform_(-0.2, 0.2)
        feat = smooth_map(bs, C, dev, seed=bs)
        g = torch.Generator().manual_seed(100 + bs)
        rois = torch.zeros((bs, n_rois, 7))
        rois[:, :, 0] = torch.rand((bs, n_rois), generator=g) * (pc_range[3] - pc_range[0]) + pc_range[0]
        rois[:, :, 1] = torch.rand((bs, n_rois), generator=g) * (pc_range[4] - pc_range[1]) + pc_range[1]
        rois[:, :, 2] = -1.0
        rois[:, :, 3:6] = torch.tensor([3.9, 1.6, 1.56]) * (0.8 + 0.4 * torch.rand((bs, n_rois, 3), generator=g))
        rois[:, :, 6] = (torch.rand((bs, n_rois), generator=g) * 2 - 1) * 3.14159
        rois = rois.to(dev)
        R = bs * n_rois
        args = (rois, feat, pc_range, VOXEL_SIZE, ratio, G)
        wpack, scale, shift = head._packed_fc()

        def per_sample():
            return first(per_sample_pool(*args).view(R, -1, 1))[:, :, 0]

        def crop():
            return first(bev_roi_ops.bev_roi_crop(*args).view(R, -1, 1))[:, :, 0]

        def fused():
            return bev_roi_ops.bev_roi_crop_fc(*args, wpack, cout, scale, shift, relu=True)

        def crop_only():
            return bev_roi_ops.bev_roi_crop(*args)
        y_a, y_b, y_c = per_sample(), crop(), fused()
        out_scale = max(1.0, float(y_a.abs().max()))
        err_b, err_c = float((y_b - y_a).abs().max()), float((y_c - y_a).abs().max())
        pool_err = float((crop_only() - per_sample_pool(*args)).abs().max())
        assert max(err_b, err_c) <= 1e-3 * out_scale, (err_b, err_c, out_scale)
        del y_a, y_b, y_c
        torch.cuda.empty_cache()
        ms_a, ms_b, ms_c, ms_crop = rounds([per_sample, crop, fused, crop_only], calls, warmup)
        pooled_bytes = R * C * G * G * 4
        res = {'bs': bs, 'rois_per_sample': n_rois, 'rois': R, 'channels': C, 'map': [H, W], 'grid_size': G, 'first_fc': cout,
               'ms_per_sample': round(ms_a, 4), 'ms_crop': round(ms_b, 4), 'ms_fused': round(ms_c, 4), 'ms_crop_only': round(ms_crop, 4),
               'crop_only_output_GBps': round(pooled_bytes / ms_crop / 1e6, 1), 'pooled_tensor_bytes': pooled_bytes,
               'fused_first_fc_TFLOPs': round(2.0 * R * C * G * G * cout / ms_c / 1e9, 2),
               'launches_per_sample': scr_tool.launches(per_sample), 'launches_crop': scr_tool.launches(crop), 'launches_fused': scr_tool.launches(fused),
               'peak_bytes_per_sample': peak_bytes(per_sample), 'peak_bytes_crop': peak_bytes(crop), 'peak_bytes_fused': peak_bytes(fused),
               'fc_chunks': bev_roi_ops.bev_roi_crop_fc_chunks(R, C, G, cout),
               'max_abs_diff_crop': err_b, 'max_abs_diff_fused': err_c, 'max_abs_diff_pooled': pool_err, 'output_scale': out_scale}
    del head, feat
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, nargs='+', default=[32, 4])
    ap.add_argument('--rois', type=int, default=100)
    ap.add_argument('--calls', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-launch-count', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'second_iou_rate.json'))
    args = ap.parse_args()
    scr_tool.COUNT_LAUNCHES = not args.no_launch_count
    dev = torch.device('cuda:0')
    runs = [run(bs, args.rois, args.calls, args.warmup, dev) for bs in args.bs]
    out = {'tool': 'tools/second_iou_rate.py', 'device': torch.cuda.get_device_name(0), 'calls': args.calls, 'warmup': args.warmup, 'runs': runs,
           'fused_beats_crop_at_every_bs': all(r['ms_fused'] < r['ms_crop'] for r in runs)}
    line = json.dumps(out)
    print(line)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()

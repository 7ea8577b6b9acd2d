"""pdm_post_process's host side without a GPU: the workspace arithmetic and argument validation (every bad call returns
non-zero with a pdm_last_error message before anything is enqueued)."""
import ctypes

import pytest


def _lib():
    from pdm_ssd_amd import _native
    return _native.lib()


def _align(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("S,pre,post", [(1, 1, 1), (32, 4096, 500), (96, 4096, 500), (3, 16384, 100), (5, 100, 1000)])
def test_workspace_bytes_arithmetic(S, pre, post):
    cb = (pre + 63) // 64
    postc = min(post, pre)
    want = (_align(S * pre * cb * 8) + _align(S * pre * 7 * 4) + 3 * _align(S * pre * 4) + 2 * _align(S * 4) +
            _align(S * postc * 4))
    assert _lib().pdm_post_process_workspace_bytes(S, pre, post) == want
    assert want >= S * pre * cb * 8


def test_workspace_bytes_of_the_issue_sizes():
    mask = 32 * 4096 * 64 * 8
    assert mask == 64 * 2 ** 20
    assert _lib().pdm_post_process_workspace_bytes(32, 4096, 500) >= mask
    assert _lib().pdm_post_process_workspace_bytes(96, 4096, 500) >= 3 * mask
    for bad in [(0, 10, 10), (-1, 10, 10), (1, 0, 10), (1, 10, 0)]:
        assert _lib().pdm_post_process_workspace_bytes(*bad) == 0


class _Args:
    """a well-formed argument list over host buffers (never dereferenced: each case below is rejected first)"""

    def __init__(self):
        self.buf = ctypes.create_string_buffer(1 << 16)
        p = ctypes.addressof(self.buf)
        self.kw = dict(B=2, C=3, multi=0, rows=100, cls=p, cls_stride=3, boxes=p, box_stride=7, offsets=p,
                       batch_index=None, score_thresh=0.1, pre=64, post=10, nms_thresh=0.1, normal=0, G=0, gt_dim=8,
                       gt=None, nt=0, thresh=None, ws=p, ws_bytes=_lib().pdm_post_process_workspace_bytes(2, 64, 10),
                       rows_out=p, boxes_out=p, scores_out=p, labels_out=p, count=p, err=p, recall=None)

    def call(self, **over):
        k = dict(self.kw, **over)
        return _lib().pdm_post_process(None, k['B'], k['C'], k['multi'], k['rows'], k['cls'], k['cls_stride'], k['boxes'],
                                       k['box_stride'], k['offsets'], k['batch_index'], k['score_thresh'], k['pre'],
                                       k['post'], k['nms_thresh'], k['normal'], k['G'], k['gt_dim'], k['gt'], k['nt'],
                                       k['thresh'], k['ws'], k['ws_bytes'], k['rows_out'], k['boxes_out'],
                                       k['scores_out'], k['labels_out'], k['count'], k['err'], k['recall'])


@pytest.mark.parametrize("over,needle", [
    (dict(B=-1), "B=-1"), (dict(C=0), "C=0"), (dict(rows=-5), "rows=-5"),
    (dict(pre=16385), "pre_max=16385"), (dict(pre=0), "pre_max=0"), (dict(post=0), "post_max=0"),
    (dict(post=-3), "post_max=-3"), (dict(multi=2), "multi_class=2"), (dict(multi=1, C=65, cls_stride=65), "65 classes"),
    (dict(cls_stride=2), "cls_stride=2"), (dict(box_stride=6), "box_stride=6"), (dict(G=-1), "gt rows"),
    (dict(G=4097), "gt rows"), (dict(nt=9), "recall thresholds"), (dict(nt=-1), "recall thresholds"),
    (dict(nt=2), "null recall thresholds"), (dict(gt="buf"), "recall buffer"), (dict(gt="buf", recall="buf", gt_dim=6), "gt_dim"),
    (dict(cls=None), "null cls"), (dict(boxes=None), "null cls"), (dict(offsets=None), "null pointer"),
    (dict(err=None), "null pointer"), (dict(count=None), "null pointer"), (dict(rows_out=None), "null pointer"),
    (dict(ws=None), "workspace"), (dict(ws_bytes=1000), "workspace of 1000 bytes"), (dict(B=70000), "segments"),
])
def test_bad_arguments_are_rejected_before_any_launch(over, needle):
    a = _Args()
    p = ctypes.addressof(a.buf)
    over = {k: (p if v == "buf" else v) for k, v in over.items()}
    if 'ws_bytes' in over:
        over['ws_bytes'] = a.kw['ws_bytes'] - 1 if over['ws_bytes'] == 1000 else over['ws_bytes']
        needle = "workspace of %d bytes" % over['ws_bytes']
    rc = a.call(**over)
    assert rc != 0
    msg = _lib().pdm_last_error().decode()
    assert needle in msg, msg

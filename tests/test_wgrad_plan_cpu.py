"""CPU: the contract of the weight gradient's workspace queries that the extension relies on (csrc/torch_ext.cpp asks the f16x3 query
whether the split-precision forms cover a layer: 0 = no, fall back to the fp32 form).  A query touches no pointer and makes no HIP call."""

RECORD = 9 * 1024 * 4          # one workgroup's partial tiles: 9 taps x 16 x 64 floats


def _dims(size, ci, co, k, stride=1, pad=None, dil=1, batch=2):
    d, h, w = size
    kd, kh, kw = k
    pad = pad if pad is not None else tuple(dil * (x // 2) for x in k)
    out = tuple((n + 2 * p - dil * (x - 1) - 1) // stride + 1 for n, p, x in zip(size, pad, k))
    return (batch, d, h, w, ci, *out, co, kd, kh, kw, stride, *pad, dil, dil, dil, 0)


def test_f16x3_query_says_which_layers_the_form_covers(lib):
    q = lib.osa_conv3d_wgrad_f16x3_workspace_bytes
    assert q(*_dims((6, 17, 23), 32, 32, (3, 3, 3), dil=2)) == 0            # dilated
    assert q(*_dims((1, 17, 23), 32, 32, (1, 5, 5))) == 0                   # unit stride, 5 x 5
    answers = [q(*_dims((6, 17, 23), 32, 32, (3, 3, 3))),                   # unit stride 3 x 3 x 3
               q(*_dims((6, 17, 23), 32, 32, (3, 3, 3), stride=2)),         # stride 2 (class mode)
               q(*_dims((6, 17, 23), 64, 128, (3, 3, 3))),                  # eight channel-tile pairs
               q(*_dims((1, 17, 23), 64, 64, (1, 3, 3))),
               lib.osa_conv3d_wgrad_workspace_bytes(*_dims((6, 17, 23), 32, 32, (3, 3, 3), stride=2)),
               lib.osa_conv3d_wgrad_workspace_bytes(*_dims((1, 17, 23), 32, 32, (1, 5, 5)))]
    for n in answers:
        assert n > 0 and n % RECORD == 0, n


def test_queries_refuse_kernels_their_tables_cannot_hold(lib):
    """More than two kernel indices of one parity per dimension (stride 2) and more than 16 d offsets (unit stride) are refused, not
    written past the tables."""
    assert lib.osa_conv3d_wgrad_workspace_bytes(1, 20, 8, 8, 32, 6, 4, 4, 32, 9, 1, 1, 2, 0, 0, 0, 1, 1, 1, 0) == 0
    assert b"out of the supported range" in lib.osa_last_error()
    assert lib.osa_conv3d_wgrad_workspace_bytes(1, 16, 8, 8, 32, 8, 4, 4, 32, 5, 1, 1, 2, 4, 0, 0, 2, 1, 1, 0) == 0        # k = 5, dilation 2, stride 2
    assert b"out of the supported range" in lib.osa_last_error()
    assert lib.osa_conv3d_wgrad_f16x3_workspace_bytes(1, 24, 8, 8, 32, 24, 8, 8, 32, 17, 1, 1, 1, 8, 0, 0, 1, 1, 1, 0) == 0
    assert b"more than 16 tap groups" in lib.osa_last_error()

"""CPU: the output-plane-walking transposed convolution (csrc/conv_deconv_walk.h), restated and executed.

* Tap enumeration.  For k = 3, s = 2, p = 1, op = 1 output plane 2a takes kd = 1 from input plane a; plane 2a + 1 takes kd = 2 from plane a and
  kd = 0 from plane a + 1; rows and columns alike, which makes the (kh, kw) taps of a source plane fall into the four (h, w) parity classes.
  Applied with plain einsum the enumeration must equal F.conv_transpose3d, and it must use each of the 27 taps of every input voxel once.
* The host's table of stream indices (launch_conv_deconv_walk_t: ConvArgs::toff from cls_end / td / th / tw of the class-major packed stream).
* The plane-buffer / weight-ring protocol of the kernel's pass loop, executed with an in-order vmcnt queue: no transfer overwrites a slot
  that a later step still reads (or the transpose tiles of an epilogue that has not run yet), and every operand has been waited for by its
  issuing wave and published by a barrier before its first read.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F


# ---------------------------------------------------------------- the walk's tap enumeration
def source_planes(par_d):
    """the kernel's passes of an output plane: (input plane offset, kd); an even plane has one source plane, an odd plane two"""
    return [(0, 1)] if par_d == 0 else [(0, 2), (1, 0)]


def step_taps(kh):
    """one step of a pass = kernel row kh: [(kw, class = ph * 2 + pw, dh, dw)] exactly as conv_deconv_walk_kernel's taps<KH>"""
    ph, dh = (1 if kh != 1 else 0), (1 if kh == 0 else 0)
    return [(kw, ph * 2 + (1 if kw != 1 else 0), dh, (1 if kw == 0 else 0)) for kw in range(3)]


def walk_conv_transpose(x, w):
    """x [B, Ci, D, H, W], w [Ci, Co, 3, 3, 3] -> [B, Co, 2D, 2H, 2W] by the walk: output plane -> source planes -> steps -> taps -> classes"""
    B, Ci, D, H, W = x.shape
    Co = w.shape[1]
    xp = F.pad(x, (0, 1, 0, 1, 0, 1))                                 # the zero halo on the high side (plane D, row H, column W)
    y = torch.zeros(B, Co, 2 * D, 2 * H, 2 * W, dtype=x.dtype)
    used = {}
    for od in range(2 * D):
        a = od >> 1
        acc = [torch.zeros(B, Co, H, W, dtype=x.dtype) for _ in range(4)]
        for dd, kd in source_planes(od & 1):
            if a + dd >= D:                                           # plane D does not exist: the kernel skips the pass
                for kh in range(3):
                    for kw, _, _, _ in step_taps(kh):
                        used[(od & 1, kd, kh, kw)] = used.get((od & 1, kd, kh, kw), 0)
                continue
            for kh in range(3):
                for kw, cls, dh, dw in step_taps(kh):
                    acc[cls] += torch.einsum("bihw,io->bohw", xp[:, :, a + dd, dh:dh + H, dw:dw + W], w[:, :, kd, kh, kw])
                    used[(od & 1, kd, kh, kw)] = used.get((od & 1, kd, kh, kw), 0) + 1
        for cls in range(4):
            y[:, :, od, (cls >> 1)::2, (cls & 1)::2] = acc[cls]
    return y, used


@pytest.mark.parametrize("shape", [(1, 3, 1, 2, 3), (2, 4, 2, 3, 5), (1, 2, 5, 4, 4)], ids=["D1", "D2", "D5"])
def test_walk_enumeration_equals_conv_transpose3d(shape):
    B, Ci, D, H, W = shape
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, Ci, D, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Ci, 5, 3, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1)
    got, _ = walk_conv_transpose(x, w)
    assert got.shape == ref.shape
    torch.testing.assert_close(got, ref, atol=1e-12, rtol=1e-12)


def test_every_tap_of_every_input_voxel_is_used_exactly_once():
    """(kd, kh, kw) -> exactly one (output plane parity, source plane, step, class); an input voxel (d, h, w) therefore contributes through each
    of its 27 taps to exactly one output voxel, (2 (d - dd) + par, 2 (h - dh) + ph, 2 (w - dw) + pw) = (2d - 1 + kd, 2h - 1 + kh, 2w - 1 + kw)."""
    seen = {}
    for par in (0, 1):
        for dd, kd in source_planes(par):
            for kh in range(3):
                for kw, cls, dh, dw in step_taps(kh):
                    assert (kd, kh, kw) not in seen, f"tap {(kd, kh, kw)} enumerated twice"
                    seen[(kd, kh, kw)] = (par, dd, cls, dh, dw)
    assert sorted(seen) == sorted(itertools.product(range(3), repeat=3))
    for (kd, kh, kw), (par, dd, cls, dh, dw) in seen.items():
        # input voxel i reaches output 2 (i - off) + parity, which conv_transpose3d defines as 2 i - pad + k
        assert (-2 * dd + par, -2 * dh + (cls >> 1), -2 * dw + (cls & 1)) == (kd - 1, kh - 1, kw - 1)
    # counted on a tensor: every (parity, tap) is applied once per output plane of that parity, except kd = 0 at the last odd plane (plane D is zero)
    D = 3
    _, used = walk_conv_transpose(torch.zeros(1, 1, D, 2, 2, dtype=torch.float64), torch.zeros(1, 1, 3, 3, 3, dtype=torch.float64))
    for (par, kd, kh, kw), n in used.items():
        assert n == (D - 1 if kd == 0 else D)
    assert len(used) == 27


# ---------------------------------------------------------------- the host's stream-index table
def class_major_stream():
    """csrc/conv3d.hip deconv_taps(k = 3, pad = 1): per class c = (pd, ph, pw) the taps that hit real inputs, (kz, ky, kx, dz, dy, dx), and cls_end"""
    def dim(par):                                                      # deconv_dim_taps: kernel indices in ascending order
        out = []
        for t in range(3):
            num = par + 1 - t
            if num % 2 == 0:
                out.append((num // 2 if num >= 0 else -((-num) // 2), t))
        return out
    taps, cls_end = [], []
    for c in range(8):
        for (dz, kz), (dy, ky), (dx, kx) in itertools.product(dim((c >> 2) & 1), dim((c >> 1) & 1), dim(c & 1)):
            taps.append((kz, ky, kx, dz, dy, dx))
        cls_end.append(len(taps))
    return taps, cls_end


def test_stream_index_table_of_the_launcher():
    taps, cls_end = class_major_stream()
    assert len(taps) == 27 and cls_end == [1, 3, 5, 9, 11, 15, 19, 27]
    toff, c = {}, 0
    for t, (kz, ky, kx, dz, dy, dx) in enumerate(taps):                # launch_conv_deconv_walk_t: from the class and the input offsets alone
        while t >= cls_end[c]:
            c += 1
        kd = (0 if dz == 1 else 2) if (c >> 2) & 1 else 1
        kh = (0 if dy == 1 else 2) if (c >> 1) & 1 else 1
        kw = (0 if dx == 1 else 2) if c & 1 else 1
        assert (kd, kh, kw) == (kz, ky, kx), "the table would fetch another tap's weights"
        toff[kd * 9 + kh * 3 + kw] = t
    assert sorted(toff) == list(range(27)) and sorted(toff.values()) == list(range(27))
    # the walk's classes and offsets are the stream's
    for kh in range(3):
        for kw, cls, dh, dw in step_taps(kh):
            for dd, kd in source_planes(0) + source_planes(1):
                kz, ky, kx, dz, dy, dx = taps[toff[kd * 9 + kh * 3 + kw]]
                assert (dz, dy, dx) == (dd, dh, dw)
                c = next(i for i, e in enumerate(cls_end) if toff[kd * 9 + kh * 3 + kw] < e)
                assert c & 3 == cls and (c >> 2) == (0 if kd == 1 else 1)


# ---------------------------------------------------------------- plane buffers and weight ring: the pass loop, executed
GEO = {1: dict(NIB=2, NP=6), 2: dict(NIB=3, NP=4)}                    # DeconvWalkGeo<WN>: B transfers per wave and step, plane pieces per wave and pass


def run_protocol(WN, nch, Di, o0, o1, slack=0):
    NIB, NP = GEO[WN]["NIB"], GEO[WN]["NP"]
    nsrc = lambda od: (2 if (od >> 1) + 1 < Di else 1) if od & 1 else 1
    kd_of = lambda od, j: (2 if j == 0 else 0) if od & 1 else 1
    passes = [(od, j, c) for od in range(o0, o1) for j in range(nsrc(od)) for c in range(nch)]
    steps = [(od, j, c, k) for (od, j, c) in passes for k in range(3)]
    # LDS resources: ("ring", slot) / ("plane", buf) -> what they hold; transfers in flight in issue order (one wave's vmcnt queue; every wave
    # issues the same instruction counts and runs the same waits, so one queue stands for all of them)
    holds, status = {}, {}                                            # status: "flight" -> "home" (issuer waited) -> "pub" (barrier after that)
    queue = []                                                        # one entry PER INSTRUCTION: (resource, transfer id) -- vmcnt counts instructions
    latest = {}                                                       # resource -> id of the transfer that wrote it last
    last_read = {}

    def issue(res, what, n, now):
        assert last_read.get(res, -2) < now, f"{res}: overwritten at step {now} while step {last_read.get(res)} reads it"
        holds[res], status[res] = what, "flight"
        latest[res] = latest.get(res, 0) + 1
        queue.extend([(res, latest[res])] * n)

    def wait(n_left):                                                 # s_waitcnt vmcnt(n_left): the oldest instructions complete until n_left remain
        del queue[:max(0, len(queue) - n_left)]
        for res in status:
            if status[res] == "flight" and (res, latest[res]) not in queue:     # home only when EVERY instruction of its last transfer is
                status[res] = "home"

    def barrier():
        for res, s in status.items():
            if s == "home":
                status[res] = "pub"

    def read(res, what, now):
        assert holds.get(res) == what, f"step {now}: {res} holds {holds.get(res)}, expected {what}"
        assert status[res] == "pub", f"step {now}: {res} read while {status[res]}"
        last_read[res] = now

    look = [0]

    def issue_b(slot, now):                                           # the look-ahead iterator: past the end it stays on the last step
        s = steps[min(look[0], len(steps) - 1)]
        issue(("ring", slot), ("B", s[0], kd_of(s[0], s[1]), s[2], s[3]), NIB, now)
        look[0] += 1

    # prologue
    issue(("plane", 0), ("P", passes[0]), NP, -1)
    issue_b(0, -1)
    issue_b(1, -1)
    wait(0)
    t, slot = 0, 0
    for q, (od, j, c) in enumerate(passes):
        cur = q & 1
        nxt = passes[q + 1] if q + 1 < len(passes) else None
        for k in range(3):
            barrier()
            issue_b((slot + 2) % 3, t)
            if k == 0:
                issue(("plane", cur ^ 1), ("P", nxt), NP, t)
            read(("ring", slot), ("B", od, kd_of(od, j), c, k), t)
            read(("plane", cur), ("P", (od, j, c)), t)
            wait((NIB + NP if k <= 1 else NIB) + slack)
            slot, t = (slot + 1) % 3, t + 1
        if (j, c) == (nsrc(od) - 1, nch - 1):                         # the output plane is complete: barrier, transpose tiles in buffer `cur`
            barrier()
            assert not any(r == ("plane", cur) for r, _ in queue), "a transfer is in flight into the buffer the epilogue's tiles alias"
            holds[("plane", cur)], status[("plane", cur)] = ("tiles", od), "pub"
            last_read[("plane", cur)] = t - 1                         # (the tiles are dead once the wave is past the next barrier)
    wait(0)
    assert not queue
    return len(steps)


@pytest.mark.parametrize("WN", [1, 2])
@pytest.mark.parametrize("nch", [1, 2, 4, 8])
@pytest.mark.parametrize("seg", [(6, 0, 1), (6, 1, 2), (6, 0, 2), (6, 1, 3), (6, 0, 12), (6, 3, 12), (6, 11, 12), (6, 10, 12), (1, 0, 2), (1, 1, 2), (2, 0, 4), (12, 5, 17)],
                         ids=lambda s: f"Di{s[0]}-planes{s[1]}..{s[2] - 1}")
def test_plane_buffer_and_weight_ring_protocol(WN, nch, seg):
    Di, o0, o1 = seg
    n = run_protocol(WN, nch, Di, o0, o1)
    # an even plane is 3 steps per chunk, an odd plane 6 -- 3 where its upper neighbour plane does not exist
    want = sum(3 * nch * ((2 if (od >> 1) + 1 < Di else 1) if od & 1 else 1) for od in range(o0, o1))
    assert n == want


@pytest.mark.parametrize("WN", [1, 2])
def test_the_model_catches_a_wait_that_is_one_instruction_short(WN):
    """vmcnt immediates one too large leave the last instruction of the next step's weights (or of the next plane) in flight at its first read"""
    with pytest.raises(AssertionError, match="read while flight"):
        run_protocol(WN, 2, 6, 0, 4, slack=1)

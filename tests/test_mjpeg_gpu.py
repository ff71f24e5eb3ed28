"""s2v_jpeg_encode (csrc/jpeg.hip), mjpeg.JpegEncoder and the CLI's --outfile NAME.avi on the device.

Bar: BYTE-EQUAL.  The stream contract is integer arithmetic, so out[b, :sizes[b]] equals the NumPy restatement
(mjpeg_cases.restate) byte for byte, with status 0; test_mjpeg_host proves those streams decode and that the case
list reaches every branch of the entropy coder.  The bytes after the last slot are filled with a sentinel first and
must still hold it."""
import json
import struct

import numpy as np
import pytest
import torch

import mjpeg_cases as MC
import s2v_import  # noqa: F401
from helpers import write_mp4_header, write_wav

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0xA5
PAD = 4096                                                                 # bytes past the last slot


def encode(frames, quality, order, capacity=None):
    """One s2v_jpeg_encode launch over uint8 [n, h, w, 3] (NumPy) -> (slots uint8 [n, capacity], sizes, status),
    after checking the bytes past the last slot."""
    from s2v_amd import _lib, mjpeg
    lib = _lib.load()
    frames = np.ascontiguousarray(frames, np.uint8)
    n, h, w = frames.shape[:3]
    head = mjpeg.jfif_header(h, w, quality)
    capacity = capacity or len(head) + lib.s2v_jpeg_worst_bytes(h, w)
    d_frames = torch.from_numpy(frames).to(DEV)
    d_head = torch.from_numpy(np.frombuffer(head, np.uint8).copy()).to(DEV)
    d_qt = torch.from_numpy(mjpeg.quant_tables(quality).astype(np.int16)).to(DEV)
    out = torch.full((n * capacity + PAD,), SENTINEL, dtype=torch.uint8, device=DEV)
    sizes = torch.full((n,), -5, dtype=torch.int32, device=DEV)
    status = torch.full((n,), -5, dtype=torch.int32, device=DEV)
    ws_bytes = lib.s2v_jpeg_ws_bytes(n, h, w)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.s2v_jpeg_encode(d_frames.data_ptr(), n, h, w, 3 * w, 3 * w * h, 1 if order == "bgr" else 0,
                                   d_head.data_ptr(), len(head), d_qt.data_ptr(), out.data_ptr(), capacity,
                                   sizes.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes,
                                   torch.cuda.current_stream().cuda_stream), "s2v_jpeg_encode")
    ho = out.cpu().numpy()
    assert (ho[n * capacity:] == SENTINEL).all()
    return ho[: n * capacity].reshape(n, capacity), sizes.cpu().tolist(), status.cpu().tolist()


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return int(d[0]) if len(d) else n


def assert_stream(slot, size, status, exp):
    assert status == 0 and size == len(exp), (status, size, len(exp))
    got = slot[:size].tobytes()
    assert got == exp, f"first difference at byte {first_difference(got, exp)} of {len(exp)}"


@pytest.mark.parametrize("c", MC.CASES, ids=MC.case_id)
def test_bytes_equal_the_restatement(c):
    kind, h, w, quality, order = c
    exp, _ = MC.restate_case(c)
    slots, sizes, status = encode(MC.image(kind, h, w)[None], quality, order)
    assert_stream(slots[0], sizes[0], status[0], exp)


def test_three_frames_in_one_launch():
    frames = np.stack([MC.image("mixed", 150, 43, seed=s) for s in (0, 1, 2)])
    slots, sizes, status = encode(frames, 95, "bgr")
    exps = [MC.restate(f, 95, "bgr")[0] for f in frames]
    assert len({len(e) for e in exps}) == 3                                # three different streams
    for b in range(3):
        assert_stream(slots[b], sizes[b], status[b], exps[b])


def test_cropped_view_is_encoded_where_it_lies():
    from s2v_amd import mjpeg
    big = np.stack([MC.image("mixed", 60, 90, seed=s) for s in (3, 4)])
    d_big = torch.from_numpy(big).to(DEV)
    view = d_big[:, 5:42, 7:57]                                            # 37 x 50 at pitch 270 > 150
    assert view.stride() == (60 * 90 * 3, 270, 3, 1) and not view.is_contiguous()
    enc = mjpeg.JpegEncoder(37, 50, quality=95, order="rgb", device=DEV)
    out, sizes, status = enc.encode(view)
    assert out.shape == (2, enc.capacity) and enc.capacity == len(enc.header) + 65536
    for b in range(2):
        exp, _ = MC.restate(big[b, 5:42, 7:57], 95, "rgb")
        assert_stream(out[b].cpu().numpy(), int(sizes[b]), int(status[b]), exp)
    # a view the kernel cannot address (channels reversed) is copied first, with the same answer as its copy
    flipped = d_big[:, :37, :50].flip(3)
    out, sizes, status = enc.encode(flipped)
    exp, _ = MC.restate(big[0, :37, :50, ::-1], 95, "rgb")
    assert_stream(out[0].cpu().numpy(), int(sizes[0]), int(status[0]), exp)


def test_overflow_reports_the_size_and_leaves_the_neighbours():
    frames = np.stack([MC.image(k, 48, 64) for k in ("smooth", "noise", "zeros", "noise")])
    frames[3] = frames[3][::-1].copy()
    exps = [MC.restate(f, 100, "rgb")[0] for f in frames]
    lens = [len(e) for e in exps]
    capacity = max(lens[0], lens[2]) + 7                                   # an odd capacity: unaligned slots
    assert lens[1] > capacity and lens[3] > capacity
    slots, sizes, status = encode(frames, 100, "rgb", capacity=capacity)
    assert status == [0, 1, 0, 1] and sizes == lens
    assert_stream(slots[0], sizes[0], status[0], exps[0])
    assert_stream(slots[2], sizes[2], status[2], exps[2])
    # exactly enough is enough; one byte less is not
    for cap, st in ((lens[1], 0), (lens[1] - 1, 1)):
        slots, sizes, status = encode(frames[1:2], 100, "rgb", capacity=cap)
        assert status == [st] and sizes == [lens[1]]
        if st == 0:
            assert_stream(slots[0], sizes[0], status[0], exps[1])


def test_encode_to_host_retries_a_frame_that_does_not_fit():
    from s2v_amd import mjpeg
    frames = np.stack([MC.image("noise", 48, 64), MC.image("zeros", 48, 64), MC.image("mixed", 48, 64)])
    exps = [MC.restate(f, 100, "bgr")[0] for f in frames]
    enc = mjpeg.JpegEncoder(48, 64, quality=100, order="bgr", device=DEV)
    d = torch.from_numpy(frames).to(DEV)
    assert enc.encode_to_host(d) == exps                                   # the default capacity holds them
    enc.capacity = len(exps[1]) + 40                                       # forced small: only the flat frame fits
    _, sizes, status = enc.encode(d)
    assert status.tolist() == [1, 0, 1] and sizes.tolist() == [len(e) for e in exps]
    assert enc.encode_to_host(d) == exps
    assert enc.encode_to_host(d[:1]) == exps[:1]                           # nothing fits: every frame retried


def test_bad_arguments_are_refused():
    from s2v_amd import _lib, mjpeg
    lib = _lib.load()
    t = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = t.data_ptr()
    ws = torch.zeros(lib.s2v_jpeg_ws_bytes(1, 16, 16), dtype=torch.uint8, device=DEV)
    good = dict(frames=p, n=1, h=16, w=16, pitch=48, stride=768, bgr=1, header=p, hb=600, qt=p, out=p, cap=4096,
                sizes=p, status=p, ws=ws.data_ptr(), wsb=ws.numel())
    for bad in (dict(frames=None), dict(out=None), dict(ws=None), dict(n=0), dict(h=0), dict(w=70000), dict(pitch=47),
                dict(bgr=2), dict(hb=0), dict(cap=0), dict(wsb=ws.numel() - 1), dict(ws=ws.data_ptr() + 1)):
        a = dict(good, **bad)
        rc = lib.s2v_jpeg_encode(a["frames"], a["n"], a["h"], a["w"], a["pitch"], a["stride"], a["bgr"], a["header"],
                                 a["hb"], a["qt"], a["out"], a["cap"], a["sizes"], a["status"], a["ws"], a["wsb"],
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == -1 and b"jpeg_encode" in lib.s2v_last_error(), bad
    assert lib.s2v_jpeg_worst_bytes(16, 16) == 6 * 416 + 2 and lib.s2v_jpeg_ws_bytes(0, 16, 16) == 0
    enc = mjpeg.JpegEncoder(16, 16, device=DEV)
    with pytest.raises(ValueError):
        enc.encode(torch.zeros((1, 16, 17, 3), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        mjpeg.JpegEncoder(16, 16, order="gbr", device=DEV)


def test_cli_writes_a_motion_jpeg_avi(tmp_path, capsys):
    """The 8-frame synthetic-weight run: with --outfile o.npz the arrays, as before; with --outfile x.avi eight 00dc
    chunks byte-equal to the restatement of those frames, the header's fps that of meta, the input audio beside
    them."""
    from s2v_amd import inference, mjpeg
    mp4 = write_mp4_header(tmp_path / "v.mp4", 200, 180, 12, 12800, 6144)              # 25 fps
    wav = write_wav(tmp_path / "a.wav", rate=16000, channels=1, seconds=0.5)
    args = ["--face", str(mp4), "--audio", str(wav), "--max_frames", "8", "--outfile"]
    npz = tmp_path / "o.npz"
    assert inference.main(args + [str(npz)]) == 0
    z = np.load(npz)
    frames = z["frames"]
    assert sorted(z.files) == ["frames", "preds"] and frames.shape == (8, 180, 200, 3)
    last = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "video_bytes" not in last and "jpeg_quality" not in last and last["outfile"] == str(npz)
    avi = tmp_path / "out" / "x.avi"
    assert inference.main(args + [str(avi)]) == 0
    meta = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    data = avi.read_bytes()
    assert meta["video_bytes"] == len(data) and meta["jpeg_quality"] == 95 and meta["frames"] == 8
    assert {k: v for k, v in meta.items() if k in last and k not in ("seconds", "outfile")} == \
        {k: v for k, v in last.items() if k not in ("seconds", "outfile")}
    chunks, movi = MC.riff_walk(data)
    video = [data[o:o + s] for p, c, o, s in chunks if p == (b"movi",) and c == b"00dc"]
    audio = b"".join(data[o:o + s] for p, c, o, s in chunks if p == (b"movi",) and c == b"01wb")
    assert len(video) == 8
    for i in range(8):
        exp, _ = MC.restate(frames[i], 95, "bgr")
        assert video[i] == exp, f"frame {i}: first difference at byte {first_difference(video[i], exp)}"
    strh = [data[o:o + s] for p, c, o, s in chunks if p == (b"hdrl", b"strl") and c == b"strh"]
    assert len(strh) == 2 and strh[0][:8] == b"vidsMJPG" and strh[1][:4] == b"auds"
    scale, rate = struct.unpack("<II", strh[0][20:28])
    assert rate / scale == meta["fps"] == 25.0
    pcm, wav_rate = mjpeg.wav_pcm16(str(wav))
    assert wav_rate == 16000 and audio == MC.pcm_reference(pcm, 16000, 8, rate, scale).tobytes()
    assert len(audio) == 2 * 8 * 16000 // 25
    # the same frames in encoder batches of 3, 3 and 2, at another quality through the flag's path
    again = tmp_path / "y.avi"
    dev = torch.from_numpy(frames).to(DEV)
    assert inference.write_avi(str(again), dev, meta["fps"], str(wav), 95, batch=3) == len(data)
    assert again.read_bytes() == data
    with pytest.raises(SystemExit):
        inference.main(args + [str(avi), "--jpeg_quality", "0"])

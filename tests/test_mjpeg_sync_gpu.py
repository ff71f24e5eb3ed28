"""s2v_jpeg_decode_sync (csrc/jpeg_dec.hip, jpeg_entropy_decode_sync), mjpeg.JpegDecoder(split="sync" / "auto") and the
CLI's --jpeg_decode on the device.

Bar: EQUALITY, as for s2v_jpeg_decode: every pixel equals Pillow's with status 0, at 4 and 64 bytes a subsequence and
at the default; test_mjpeg_sync_host proves that these streams at these sizes reach every hazard of a cut (a 0xFF
before it, a stuffed 0x00 behind it, a pass-through, blocks over three subsequences, wrong guesses of every kind,
dozens of rounds) and that the same step function passes them under AddressSanitizer on the host.  Every decode goes
into a cropped view of a sentinel-filled buffer whose margins and tail must keep the sentinel."""
import json

import numpy as np
import pytest
import torch

import mjpeg_cases as MC
import mjpeg_decode_cases as DC
import mjpeg_sync_cases as SC
import s2v_import  # noqa: F401
from helpers import write_wav

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0xA5
TOP, LEFT, BOTTOM, RIGHT, TAIL = 1, 2, 2, 3, 4096           # the margins of the sentinel buffer around a frame
SERIAL_STATUS = {"bad_code": 1, "run_past_63": 2, "truncated": 3}


def decode(files, order="rgb", split="sync", sub_bytes=None):
    """One JpegDecoder.decode of the files into a view of a sentinel buffer -> (uint8 [n, h, w, 3], status list,
    the split that ran), after checking every byte outside the view."""
    from s2v_amd import mjpeg
    info = mjpeg.parse_jpeg(files[0])
    n, h, w = len(files), info.h, info.w
    H, W = h + TOP + BOTTOM, w + LEFT + RIGHT
    flat = torch.full((n * H * W * 3 + TAIL,), SENTINEL, dtype=torch.uint8, device=DEV)
    view = flat[: n * H * W * 3].view(n, H, W, 3)[:, TOP:TOP + h, LEFT:LEFT + w]
    dec = mjpeg.JpegDecoder(h, w, info.sampling, order=order, device=DEV, split=split, sub_bytes=sub_bytes)
    out, status = dec.decode(files, out=view)
    assert out.data_ptr() == view.data_ptr()
    host = flat.cpu().numpy()
    assert (host[n * H * W * 3:] == SENTINEL).all()
    box = host[: n * H * W * 3].reshape(n, H, W, 3)
    outside = np.ones((H, W), bool)
    outside[TOP:TOP + h, LEFT:LEFT + w] = False
    assert (box[:, outside] == SENTINEL).all()
    return box[:, TOP:TOP + h, LEFT:LEFT + w].copy(), status.cpu().tolist(), dec.picked


def assert_pixels(got, data, order):
    exp = DC.pillow_pixels(data)
    exp = exp[..., ::-1] if order == "bgr" else exp
    assert got.shape == exp.shape
    assert np.array_equal(got, exp), f"{int((got != exp).any(axis=2).sum())} of {exp.shape[0] * exp.shape[1]} pixels differ"


@pytest.mark.parametrize("sub", [4, 64, None], ids=["sub4", "sub64", "default"])
@pytest.mark.parametrize("k", range(len(SC.CASES)), ids=[DC.case_id(c) for c in SC.CASES])
def test_pixels_equal_pillow(k, sub):
    data = DC.pillow_file(SC.CASES[k])
    order = ("rgb", "bgr")[k % 2]
    px, status, picked = decode([data], order, "sync", sub)
    assert status == [0] and picked == "sync"
    assert_pixels(px[0], data, order)


def test_the_tall_stream_takes_more_than_one_pass():
    """at the default sub_bytes the tall noise stream has more subsequences than the workgroup has lanes"""
    from s2v_amd import mjpeg
    data = DC.pillow_file(SC.TALL_CASES[0])
    s, e = mjpeg.parse_jpeg(data).scan
    assert (e - s) / mjpeg.SYNC_SUB_BYTES > 1024


@pytest.mark.parametrize("sub", [4, 64, None], ids=["sub4", "sub64", "default"])
def test_four_frames_with_three_table_sets_in_one_call(sub):
    from s2v_amd import mjpeg
    files = [DC.pillow_file(("mixed", 150, 43, 2, r, q, o)) for r, q, o in
             (("none", 75, False), ("none", 5, True), ("none", 100, True), ("none", 75, False))]
    cnt = mjpeg.pack_streams(files, 150, 43, 2)[2]
    assert cnt["sets"] == 3 and cnt["intervals"] == 4 and len({len(f) for f in files}) == 3
    px, status, _ = decode(files, "bgr", "sync", sub)
    assert status == [0, 0, 0, 0]
    for k, f in enumerate(files):
        assert_pixels(px[k], f, "bgr")


@pytest.mark.parametrize("sub", [4, 64, None], ids=["sub4", "sub64", "default"])
@pytest.mark.parametrize("how", DC.CORRUPTIONS)
def test_a_damaged_stream_marks_its_frame_only(how, sub):
    """The same three streams pass tools/jpeg_sync_host.cpp under AddressSanitizer (test_mjpeg_sync_host)."""
    good = [DC.pillow_file(DC.CORRUPT_BASE), DC.pillow_file(("mixed",) + DC.CORRUPT_BASE[1:])]
    px, status, _ = decode([good[0], DC.corrupt(good[0], how), good[1]], "rgb", "sync", sub)
    assert status == [0, SERIAL_STATUS[how], 0]
    assert_pixels(px[0], good[0], "rgb")
    assert_pixels(px[2], good[1], "rgb")


@pytest.mark.parametrize("how", DC.CORRUPTIONS)
def test_a_damaged_stream_without_restart_markers(how):
    """one interval a frame: the status is the serial decoder's (split 0) on the same damage"""
    base = ("noise", 40, 56, 2, "none", 75, False)
    good = DC.pillow_file(base)
    p = DC.parse(good)
    s, e = p["scan"]
    if how == "truncated":
        cut = s + (e - s) // 2
        bad = good[:cut - (good[cut - 1] == 0xFF)] + good[e:]
    elif how == "bad_code":
        at = next(a for a in range(s + (e - s) // 4, e - 18) if 0xFF not in good[a - 1:a + 17])
        bad = good[:at] + b"\xff\x00" * 8 + good[at + 16:]
    else:
        bits = "00" + "11111111001" * 4                                  # Annex K luma: DC category 0, AC 0xF0
        bits += "1" * (-len(bits) % 8)
        bad = good[:s] + int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00") + good[e:]
    _, serial, _ = decode([good, bad, good], "rgb", 0)
    assert serial == [0, SERIAL_STATUS[how], 0]
    for sub in (4, 64, None):
        px, status, _ = decode([good, bad, good], "rgb", "sync", sub)
        assert status == serial, sub
        assert_pixels(px[0], good, "rgb")
        assert_pixels(px[2], good, "rgb")


@pytest.mark.parametrize("c", DC.OWN_CASES, ids=MC.case_id)
def test_sync_equals_wave_on_the_encoder_s_streams(c):
    kind, h, w, quality, order = c
    data, _ = MC.restate(MC.image(kind, h, w), quality, order)
    wave, st_w, _ = decode([data], order, "wave")
    assert st_w == [0]
    for sub in (4, 64, None):
        sync, st_s, _ = decode([data], order, "sync", sub)
        assert st_s == [0] and np.array_equal(sync, wave), sub
    assert_pixels(wave[0], data, order)


def test_auto_picks_sync_for_long_intervals_only():
    from s2v_amd import mjpeg
    tall = DC.pillow_file(SC.TALL_CASES[0])                              # no restart markers: one interval of 270 KB
    px, status, picked = decode([tall], "rgb", "auto")
    assert picked == "sync" and status == [0]
    assert_pixels(px[0], tall, "rgb")
    for c in DC.OWN_CASES[:2]:                                           # the project's own: an interval per MCU row
        kind, h, w, quality, order = c
        data, _ = MC.restate(MC.image(kind, h, w), quality, order)
        longest = mjpeg.pack_streams([data], h, w, 2)[2]["max_interval_bytes"]
        assert longest == int(mjpeg.restart_intervals(data, mjpeg.parse_jpeg(data))[:, 1].max()) <= mjpeg.SYNC_AUTO_BYTES
        px, status, picked = decode([data], order, "auto")
        assert picked == "wave" and status == [0]
        assert_pixels(px[0], data, order)
    for name, k in (("wave", 0), ("lane", 1)):
        assert decode([tall], "rgb", name)[2] == decode([tall], "rgb", k)[2] == name
    with pytest.raises(ValueError, match="jpeg_decode"):
        mjpeg.JpegDecoder(16, 16, 2, device=DEV, split="serial")
    with pytest.raises(ValueError, match="jpeg_decode"):
        mjpeg.JpegDecoder(16, 16, 2, device=DEV, split=2)
    with pytest.raises(ValueError, match="sub_bytes"):
        mjpeg.JpegDecoder(16, 16, 2, device=DEV, split="sync", sub_bytes=6)


def test_bad_arguments_are_refused():
    from s2v_amd import _lib, mjpeg
    lib = _lib.load()
    data = DC.pillow_file(("noise", 40, 56, 2, "none", 75, False))
    buf, offs, cnt = mjpeg.pack_streams([data], 40, 56, 2)
    dev = torch.from_numpy(buf).to(DEV)
    p = dev.data_ptr()
    out = torch.zeros((40, 56, 3), dtype=torch.uint8, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    sub = 64
    nws = lib.s2v_jpeg_decode_sync_ws_bytes(1, 40, 56, 2, cnt["data_bytes"], 1, sub)
    records = cnt["data_bytes"] // sub + 2 * 1 + 2
    assert nws == lib.s2v_jpeg_decode_ws_bytes(1, 40, 56, 2) + ((48 * records + 15) & ~15)
    for bad_sub in (0, 2, 6, 8192):
        assert lib.s2v_jpeg_decode_sync_ws_bytes(1, 40, 56, 2, cnt["data_bytes"], 1, bad_sub) == 0
    assert lib.s2v_jpeg_decode_sync_ws_bytes(1, 40, 56, 3, cnt["data_bytes"], 1, sub) == 0
    ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
    good = dict(data=p + offs["data"], nb=cnt["data_bytes"], iv=p + offs["intervals"], niv=cnt["intervals"],
                ff=p + offs["frame_first"], mpf=cnt["max_per_frame"], n=1, h=40, w=56, s=2, qt=p + offs["qtables"],
                hs=p + offs["huff_sets"], ns=1, si=p + offs["set_index"], out=out.data_ptr(), pitch=168, stride=0,
                bgr=0, status=status.data_ptr(), ws=ws.data_ptr(), wsb=nws, sub=sub)

    def call(a):
        return lib.s2v_jpeg_decode_sync(a["data"], a["nb"], a["iv"], a["niv"], a["ff"], a["mpf"], a["n"], a["h"],
                                        a["w"], a["s"], a["qt"], a["hs"], a["ns"], a["si"], a["out"], a["pitch"],
                                        a["stride"], a["bgr"], a["status"], a["ws"], a["wsb"], a["sub"],
                                        torch.cuda.current_stream().cuda_stream)
    for bad in (dict(data=None), dict(iv=None), dict(ff=None), dict(qt=None), dict(hs=None), dict(si=None),
                dict(out=None), dict(ws=None), dict(status=None), dict(n=0), dict(h=0), dict(w=70000), dict(s=3),
                dict(pitch=167), dict(bgr=2), dict(sub=0), dict(sub=2), dict(sub=6), dict(sub=8192), dict(nb=0),
                dict(niv=0), dict(mpf=0), dict(ns=0), dict(wsb=nws - 1), dict(ws=ws.data_ptr() + 1)):
        assert call(dict(good, **bad)) == -1 and b"jpeg_decode" in lib.s2v_last_error(), bad
    assert call(good) == 0
    assert status.tolist() == [0] and np.array_equal(out.cpu().numpy(), DC.pillow_pixels(data))


def test_a_table_out_of_order_is_status_4():
    """two intervals handed over in descending order of offsets: every frame is suspect, nothing is written outside"""
    from s2v_amd import mjpeg
    files = [DC.pillow_file(("mixed", 40, 56, 2, "none", q, False)) for q in (75, 5)]
    buf, offs, cnt = mjpeg.pack_streams(files, 40, 56, 2)
    table = buf[offs["intervals"]:offs["intervals"] + 40].view(np.int32).reshape(2, 5)
    table[[0, 1]] = table[[1, 0]]
    dev = torch.from_numpy(buf).to(DEV)
    dec = mjpeg.JpegDecoder(40, 56, 2, device=DEV, split="sync", sub_bytes=16)
    _, status = dec.decode_packed(dev, offs, cnt)
    assert status.tolist() == [4, 4]


def test_cli_jpeg_decode_sync(tmp_path, capsys, monkeypatch):
    """--jpeg_decode sync gives the frames of --jpeg_decode wave byte for byte, on Pillow files without restart
    markers; meta records the choice; a bad value is refused before anything runs."""
    from s2v_amd import inference, mjpeg
    rgb = [MC.image("mixed", 180, 200, seed=s) for s in range(4)]
    files = [DC.pillow_encode(f, quality=90, subsampling=2, optimize=k == 2) for k, f in enumerate(rgb)]
    assert all(mjpeg.parse_jpeg(f).restart_interval == 0 for f in files)
    clip = tmp_path / "clip.avi"
    with mjpeg.AviWriter(clip, 200, 180, 25) as avi:
        for f in files:
            avi.write(f)
    wav = write_wav(tmp_path / "a.wav", rate=16000, channels=1, seconds=0.4)
    exp = np.stack([DC.pillow_pixels(f)[..., ::-1] for f in files])
    for mode in ("sync", "auto", None):
        got = inference.decode_jpeg_frames(files, DEV, batch=3, jpeg_decode=mode)
        assert np.array_equal(got.cpu().numpy(), exp), mode
    frames, metas = {}, {}
    for mode in ("wave", "sync"):
        npz = tmp_path / f"{mode}.npz"
        assert inference.main(["--face", str(clip), "--audio", str(wav), "--max_frames", "4", "--LNet_batch_size", "3",
                               "--jpeg_decode", mode, "--outfile", str(npz)]) == 0
        metas[mode] = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        frames[mode] = np.load(npz)["frames"]
    assert metas["wave"]["jpeg_decode"] == "wave" and metas["sync"]["jpeg_decode"] == "sync"
    assert metas["sync"]["frames"] == 4 and np.array_equal(frames["sync"], frames["wave"])
    with pytest.raises(SystemExit):
        inference.main(["--face", str(clip), "--audio", str(wav), "--jpeg_decode", "serial"])
    capsys.readouterr()
    with pytest.raises(ValueError, match="jpeg_decode"):
        inference.run(str(tmp_path / "missing.avi"), str(tmp_path / "missing.wav"), jpeg_decode="serial")
    monkeypatch.setenv("S2V_JPEG_DECODE", "serial")
    with pytest.raises(ValueError, match="S2V_JPEG_DECODE"):
        inference.run(str(tmp_path / "missing.avi"), str(tmp_path / "missing.wav"), jpeg_decode=None)
    monkeypatch.setenv("S2V_JPEG_DECODE", "sync")
    assert mjpeg.jpeg_decode_mode(None) == "sync" and mjpeg.jpeg_decode_mode("wave") == "wave"

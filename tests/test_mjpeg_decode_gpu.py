"""s2v_jpeg_decode (csrc/jpeg_dec.hip), mjpeg.JpegDecoder and the CLI's --face NAME.avi / NAME.jpg on the device.

Bar: EQUALITY.  The decoder is integer arithmetic that restates libjpeg-turbo's default decoder, so every pixel
equals PIL.Image.open(...).convert("RGB") (mjpeg_decode_cases.pillow_pixels), with status 0; test_mjpeg_decode_host
proves that the case list reaches every branch of the entropy decoder and that the same functions pass the damaged
streams under AddressSanitizer on the host.  Every decode here goes into a cropped view of a sentinel-filled buffer:
the bytes past every row, around every frame and past the last frame must still hold the sentinel."""
import json

import numpy as np
import pytest
import torch

import mjpeg_cases as MC
import mjpeg_decode_cases as DC
import s2v_import  # noqa: F401
from helpers import write_wav

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0xA5
TOP, LEFT, BOTTOM, RIGHT, TAIL = 1, 2, 2, 3, 4096           # the margins of the sentinel buffer around a frame


def decode(files, order="rgb", split=0):
    """One JpegDecoder.decode of the files into a view of a sentinel buffer -> (uint8 [n, h, w, 3], status list),
    after checking every byte outside the view."""
    from s2v_amd import mjpeg
    info = mjpeg.parse_jpeg(files[0])
    n, h, w = len(files), info.h, info.w
    H, W = h + TOP + BOTTOM, w + LEFT + RIGHT
    flat = torch.full((n * H * W * 3 + TAIL,), SENTINEL, dtype=torch.uint8, device=DEV)
    view = flat[: n * H * W * 3].view(n, H, W, 3)[:, TOP:TOP + h, LEFT:LEFT + w]
    dec = mjpeg.JpegDecoder(h, w, info.sampling, order=order, device=DEV, split=split)
    out, status = dec.decode(files, out=view)
    assert out.data_ptr() == view.data_ptr()
    host = flat.cpu().numpy()
    assert (host[n * H * W * 3:] == SENTINEL).all()
    box = host[: n * H * W * 3].reshape(n, H, W, 3)
    outside = np.ones((H, W), bool)
    outside[TOP:TOP + h, LEFT:LEFT + w] = False
    assert (box[:, outside] == SENTINEL).all()
    return box[:, TOP:TOP + h, LEFT:LEFT + w].copy(), status.cpu().tolist()


def expected(data, order):
    ref = DC.pillow_pixels(data)
    return ref[..., ::-1] if order == "bgr" else ref


def assert_pixels(got, data, order):
    exp = expected(data, order)
    assert got.shape == exp.shape
    assert np.array_equal(got, exp), f"{int((got != exp).any(axis=2).sum())} of {exp.shape[0] * exp.shape[1]} pixels differ"


@pytest.mark.parametrize("split", [0, 1], ids=["wave", "lane"])
@pytest.mark.parametrize("k", range(len(DC.CASES)), ids=[DC.case_id(c) for c in DC.CASES])
def test_pixels_equal_pillow(k, split):
    data = DC.pillow_file(DC.CASES[k])
    order = ("rgb", "bgr")[k % 2]
    px, status = decode([data], order, split)
    assert status == [0]
    assert_pixels(px[0], data, order)


@pytest.mark.parametrize("split", [0, 1], ids=["wave", "lane"])
@pytest.mark.parametrize("c", DC.OWN_CASES, ids=MC.case_id)
def test_the_encoder_s_streams(c, split):
    """the project's own stream contract, restated on the CPU: no encoder launch"""
    kind, h, w, quality, order = c
    data, _ = MC.restate(MC.image(kind, h, w), quality, order)
    px, status = decode([data], order, split)
    assert status == [0]
    assert_pixels(px[0], data, order)


@pytest.mark.parametrize("split", [0, 1], ids=["wave", "lane"])
def test_three_frames_with_their_own_tables(split):
    files = [DC.pillow_file(("mixed", 150, 43, 2, r, q, o)) for r, q, o in
             (("rows1", 75, False), ("none", 5, True), ("blocks3", 100, True))]
    from s2v_amd import mjpeg
    infos = [mjpeg.parse_jpeg(f) for f in files]
    assert len({i.huffman for i in infos}) == 3 and len({i.qtables.tobytes() for i in infos}) == 3
    assert mjpeg.pack_streams(files + files[:1], 150, 43, 2)[2]["sets"] == 3     # an equal set is uploaded once
    px, status = decode(files + files[:1], "bgr", split)
    assert status == [0, 0, 0, 0]
    for k, f in enumerate(files + files[:1]):
        assert_pixels(px[k], f, "bgr")


@pytest.mark.parametrize("split", [0, 1], ids=["wave", "lane"])
@pytest.mark.parametrize("how", DC.CORRUPTIONS)
def test_a_damaged_stream_marks_its_frame_only(how, split):
    """The same three streams pass tools/jpeg_decode_host.cpp under AddressSanitizer (test_mjpeg_decode_host)."""
    good = [DC.pillow_file(DC.CORRUPT_BASE), DC.pillow_file(("mixed",) + DC.CORRUPT_BASE[1:])]
    px, status = decode([good[0], DC.corrupt(good[0], how), good[1]], "rgb", split)
    assert status[0] == 0 and status[2] == 0
    assert status[1] == {"bad_code": 1, "run_past_63": 2, "truncated": 3}[how]
    assert_pixels(px[0], good[0], "rgb")
    assert_pixels(px[2], good[1], "rgb")


def test_encoder_then_decoder_on_the_device():
    from s2v_amd import mjpeg
    frames = np.stack([MC.image("mixed", 150, 43, seed=s) for s in (0, 1)])
    enc = mjpeg.JpegEncoder(150, 43, quality=90, order="bgr", device=DEV)
    files = enc.encode_to_host(torch.from_numpy(frames).to(DEV))
    dec = mjpeg.JpegDecoder.for_file(files[0], order="bgr", device=DEV)
    assert (dec.h, dec.w, dec.sampling) == (150, 43, 2)
    out, status = dec.decode(files)
    assert status.tolist() == [0, 0] and out.shape == (2, 150, 43, 3)
    for k in range(2):
        assert_pixels(out[k].cpu().numpy(), files[k], "bgr")
    # and it is the picture that went in: nearer to its source than to the other frame or to swapped channels
    got = out.cpu().numpy().astype(int)
    for k in range(2):
        err = np.abs(got[k] - frames[k]).mean()
        assert err < np.abs(got[k] - frames[1 - k]).mean() and err < np.abs(got[k] - frames[k][..., ::-1]).mean()


def test_bad_arguments_are_refused():
    from s2v_amd import _lib, mjpeg
    lib = _lib.load()
    data = DC.pillow_file(DC.CORRUPT_BASE)
    buf, offs, cnt = mjpeg.pack_streams([data], 40, 56, 2)
    dev = torch.from_numpy(buf).to(DEV)
    p = dev.data_ptr()
    out = torch.zeros((40, 56, 3), dtype=torch.uint8, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    nws = lib.s2v_jpeg_decode_ws_bytes(1, 40, 56, 2)
    # int16 coefficients of 3 x 4 MCUs of 6 blocks, a 48 x 64 luma plane and two 24 x 32 chroma planes
    assert nws == 12 * 6 * 128 + 48 * 64 + 2 * 24 * 32 and lib.s2v_jpeg_decode_ws_bytes(1, 40, 56, 3) == 0
    ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
    good = dict(data=p + offs["data"], nb=cnt["data_bytes"], iv=p + offs["intervals"], niv=cnt["intervals"],
                ff=p + offs["frame_first"], mpf=cnt["max_per_frame"], n=1, h=40, w=56, s=2, qt=p + offs["qtables"],
                hs=p + offs["huff_sets"], ns=1, si=p + offs["set_index"], out=out.data_ptr(), pitch=168, stride=0,
                bgr=0, status=status.data_ptr(), ws=ws.data_ptr(), wsb=nws, split=0)

    def call(a):
        return lib.s2v_jpeg_decode(a["data"], a["nb"], a["iv"], a["niv"], a["ff"], a["mpf"], a["n"], a["h"], a["w"],
                                   a["s"], a["qt"], a["hs"], a["ns"], a["si"], a["out"], a["pitch"], a["stride"],
                                   a["bgr"], a["status"], a["ws"], a["wsb"], a["split"],
                                   torch.cuda.current_stream().cuda_stream)
    for bad in (dict(data=None), dict(out=None), dict(ws=None), dict(status=None), dict(n=0), dict(h=0), dict(w=70000),
                dict(s=3), dict(pitch=167), dict(bgr=2), dict(split=2), dict(nb=0), dict(niv=0), dict(mpf=0),
                dict(mpf=cnt["intervals"] + 1), dict(ns=0), dict(wsb=nws - 1), dict(ws=ws.data_ptr() + 1)):
        assert call(dict(good, **bad)) == -1 and b"jpeg_decode" in lib.s2v_last_error(), bad
    assert call(good) == 0
    assert status.tolist() == [0] and np.array_equal(out.cpu().numpy(), DC.pillow_pixels(data))
    dec = mjpeg.JpegDecoder(40, 56, 2, device=DEV)
    with pytest.raises(ValueError, match="16x16"):
        dec.decode([data, DC.pillow_file(DC.CASES[0])])
    with pytest.raises(ValueError):
        dec.decode([data], out=torch.zeros((1, 40, 57, 3), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        mjpeg.JpegDecoder(40, 56, 2, order="gbr", device=DEV)


def test_cli_reads_a_motion_jpeg_avi_and_a_still(tmp_path, capsys):
    """--face clip.avi: the frames the network pastes into are exactly Pillow's pixels, in BGR, outside the face box,
    and fps is the header's; --face one.jpg: the reference's static mode; the AVI the CLI writes reads back."""
    from s2v_amd import inference, mjpeg
    rgb = [MC.image("mixed", 180, 200, seed=s) for s in range(6)]
    files = [DC.pillow_encode(f, quality=90, subsampling=2, restart_marker_rows=k % 2, optimize=k == 2)
             for k, f in enumerate(rgb)]                                   # with and without restart markers
    clip = tmp_path / "clip.avi"
    with mjpeg.AviWriter(clip, 200, 180, 30000 / 1001) as avi:
        for f in files:
            avi.write(f)
    wav = write_wav(tmp_path / "a.wav", rate=16000, channels=1, seconds=0.5)
    exp = np.stack([DC.pillow_pixels(f)[..., ::-1] for f in files])
    got = inference.decode_jpeg_frames(files, DEV, batch=4)                # batches of 4 and 2
    assert np.array_equal(got.cpu().numpy(), exp)
    npz = tmp_path / "o.npz"
    assert inference.main(["--face", str(clip), "--audio", str(wav), "--max_frames", "5", "--LNet_batch_size", "3",
                           "--outfile", str(npz)]) == 0
    meta = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert meta["frames"] == 5 and meta["fps"] == 30000 / 1001 and meta["video"] == "avi mjpeg 200x180"
    frames = np.load(npz)["frames"]
    y1, y2, x1, x2 = meta["box"]
    keep = np.ones((180, 200), bool)
    keep[y1:y2, x1:x2] = False
    assert frames.shape == (5, 180, 200, 3) and keep.sum() > 20000
    assert np.array_equal(frames[:, keep], exp[:5][:, keep])
    # a damaged frame is named
    broken = tmp_path / "broken.avi"
    with mjpeg.AviWriter(broken, 200, 180, 25) as avi:
        for k, f in enumerate(files[:3]):
            avi.write(DC.corrupt(f, "bad_code") if k == 1 else f)
    with pytest.raises(ValueError, match="frame 1"):
        inference.main(["--face", str(broken), "--audio", str(wav), "--max_frames", "3", "--outfile", str(npz)])
    capsys.readouterr()
    # the static mode, written as an AVI that reads back
    still = tmp_path / "one.jpg"
    still.write_bytes(files[0])
    out_avi = tmp_path / "out.avi"
    assert inference.main(["--face", str(still), "--audio", str(wav), "--max_frames", "5", "--fps", "20",
                           "--outfile", str(out_avi)]) == 0
    meta = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert meta["frames"] == 5 and meta["fps"] == 20.0 and meta["video"] == "jpeg 200x180 (static)"
    r = mjpeg.AviReader(out_avi)
    assert len(r) == 5 and r.fps == 20.0 and (r.w, r.h) == (200, 180) and r.audio_rate == 16000
    back, status = mjpeg.JpegDecoder.for_file(r.frame(0), order="rgb", device=DEV).decode(r.frames())
    assert status.tolist() == [0] * 5
    back = back.cpu().numpy()
    for k in range(5):
        assert np.array_equal(back[k], DC.pillow_pixels(r.frame(k)))
    near = np.abs(back[0][keep].astype(int) - DC.pillow_pixels(files[0])[keep]).mean()
    assert near < np.abs(back[0][keep].astype(int) - DC.pillow_pixels(files[1])[keep]).mean()   # the still, not another

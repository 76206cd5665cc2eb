"""GPU: one ladder behind every way to open a JPEG source -- load_jpeg with host and with device entropy, load_resident and the CPU
store over one crafted list: Pillow's pixels, the recorded counters, one refusal text per defect from all four, a clean device after
a refused open, and the host decoder overruling the device with OK."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_open_util as OU  # noqa: E402
import jpeg_util as JU  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OPENERS = ("host-entropy", "device-entropy", "resident", "cpu")
NO_SPLIT = {"split": 0, "abandoned": 0, "rounds_max": 0}          # no segment of a 72 x 128 frame reaches TSTAR_JPEG_SPLIT_BYTES
# decode_stats, entropy_stats, entropy_split_stats of the ladder list, recorded before the openers shared their ladder
RECORDED = {
    "host-entropy": ({"device": 5, "host": 0, "pillow": 5}, {"device": 0, "host": 8}, NO_SPLIT),
    "device-entropy": ({"device": 5, "host": 0, "pillow": 5}, {"device": 5, "host": 3}, NO_SPLIT),
    "resident": ({"device": 5, "host": 0, "pillow": 5}, {"device": 5, "host": 3}, NO_SPLIT),
    "cpu": ({"device": 0, "host": 5, "pillow": 5}, {"device": 0, "host": 8}, NO_SPLIT),
}


def _need_turbo():
    if not JU.turbo():
        pytest.skip("Pillow on this machine is not built on libjpeg-turbo: its bytes are not the yardstick the byte-equality "
                    "is defined against")


def _open(opener, chunk, frames=None):
    from tstar_amd import jpeg, jpeg_resident
    src = OU.source(frames)
    if opener == "resident":
        return jpeg_resident.load_resident(src, "cuda", pool_frames=4, chunk=chunk)
    if opener == "cpu":
        return jpeg.load_jpeg(src, device="cpu", chunk=chunk)
    return jpeg.load_jpeg(src, device="cuda", chunk=chunk, entropy="device" if opener == "device-entropy" else "host")


def _stats(st):
    return st.decode_stats, st.entropy_stats, st.entropy_split_stats


@pytest.mark.parametrize("chunk", OU.CHUNKS)
def test_the_ladder_list_behind_every_opener(chunk):
    _need_turbo()
    stores = {o: _open(o, chunk) for o in OPENERS}
    for o, st in stores.items():
        print(o, chunk, _stats(st))
        assert np.array_equal(st.host_frames(range(OU.N)), OU.ladder_pixels()), o
        assert _stats(st) == RECORDED[o] and list(st.decode_stats) == ["device", "host", "pillow"], o
    res = stores["resident"]
    assert _stats(res) == _stats(stores["device-entropy"])
    assert res.pool_stats()["exceptions"] == 5 and sorted(res._pool.permanent) == list(OU.PILLOW_FRAMES)
    assert res.fetch_errors() == 0


@pytest.mark.parametrize("chunk", OU.CHUNKS)
@pytest.mark.parametrize("defect", OU.DEFECTS)
def test_every_opener_refuses_a_broken_list_with_one_text(defect, chunk):
    frames, text = OU.defects()[defect]
    for o in OPENERS:
        with pytest.raises(ValueError) as e:
            _open(o, chunk, frames)
        print(o, chunk, str(e.value))
        assert str(e.value) == text, o
        if o != "cpu":
            torch.cuda.synchronize()                                    # nothing the refused open queued is left to fault
            good = _open(o, chunk)
            assert np.array_equal(good.host_frames([2, 9]), OU.ladder_pixels()[[2, 9]]), o
            torch.cuda.synchronize()


@pytest.mark.parametrize("chunk", OU.CHUNKS)
@pytest.mark.parametrize("opener", ["device-entropy", "resident"])
def test_the_host_decoder_overrules_the_device_with_ok(opener, chunk, monkeypatch):
    """The planner's frame_status reports frame 5 (good, device-routed) refused: the host decoder returns its coefficients, one
    frame is reconstructed from them, and one frame moves from the device's entropy count to the host's."""
    _need_turbo()
    OU.refuse_frame(monkeypatch)
    st = _open(opener, chunk)
    dec, ent, spl = RECORDED[opener]
    print(opener, chunk, _stats(st))
    assert np.array_equal(st.host_frames(range(OU.N)), OU.ladder_pixels())
    assert st.decode_stats == dec and st.entropy_split_stats == spl
    assert st.entropy_stats == {"device": ent["device"] - 1, "host": ent["host"] + 1}
    if opener == "resident":
        assert st.pool_stats()["exceptions"] == 6 and OU.REFUSED_GOOD_FRAME in st._pool.permanent and st.fetch_errors() == 0

"""CPU: the JPEG open's ladder on the CPU store -- a list that meets every rung (prelude, geometry, Pillow, host-routed, refused),
the texts a broken list is refused with, and the pure parts the openers share (split counters, split threshold)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_open_util as OU  # noqa: E402
import jpeg_util as JU  # noqa: E402


def _need_turbo():
    if not JU.turbo():
        pytest.skip("Pillow on this machine is not built on libjpeg-turbo: its bytes are not the yardstick the byte-equality "
                    "is defined against")


@pytest.mark.parametrize("chunk", OU.CHUNKS)
def test_the_ladder_list_on_the_cpu_store(chunk):
    from tstar_amd import jpeg
    _need_turbo()
    st = jpeg.load_jpeg(OU.source(), device="cpu", chunk=chunk)
    assert st.decode_stats == {"device": 0, "host": 5, "pillow": 5} and list(st.decode_stats) == ["device", "host", "pillow"]
    assert st.entropy_stats == {"device": 0, "host": 8}
    assert st.entropy_split_stats == {"split": 0, "abandoned": 0, "rounds_max": 0}
    assert np.array_equal(st.frames.numpy(), OU.ladder_pixels())


def test_the_ladder_list_routes_and_host_statuses():
    from tstar_amd import jpeg
    datas = list(OU.ladder())
    assert [jpeg.probe(d)[0] for d in datas[:3]] == [jpeg.UNCOVERED, jpeg.UNCOVERED, jpeg.OK]
    geom = jpeg.probe(datas[2])[1]
    assert list(jpeg.plan_segments(datas[2:], geom).route) == OU.ROUTES
    coef = np.empty((8, jpeg._sizes(geom)[0] * 64), dtype=np.int16)
    status, _ = jpeg.entropy_batch(datas[2:], geom, coef, np.empty((8, 192), dtype=np.uint16))
    assert list(status) == OU.HOST_STATUS
    assert tuple(i for i in range(OU.N) if i < 2 or status[i - 2]) == OU.PILLOW_FRAMES


@pytest.mark.parametrize("chunk", OU.CHUNKS)
@pytest.mark.parametrize("defect", OU.DEFECTS)
def test_a_broken_list_is_refused_by_name(defect, chunk):
    from tstar_amd import jpeg
    frames, text = OU.defects()[defect]
    with pytest.raises(ValueError) as e:
        jpeg.load_jpeg(OU.source(frames), device="cpu", chunk=chunk)
    assert str(e.value) == text


def test_split_counters():
    from tstar_amd import jpeg
    sstats = {"split": 0, "abandoned": 0, "rounds_max": 0}
    jpeg.count_split(sstats, np.array([0, 3, -1, 7, 0], dtype=np.int32))
    assert sstats == {"split": 3, "abandoned": 1, "rounds_max": 7}
    jpeg.count_split(sstats, np.array([2, 0], dtype=np.int32))
    jpeg.count_split(sstats, np.zeros(0, dtype=np.int32))
    assert sstats == {"split": 4, "abandoned": 1, "rounds_max": 7}


def test_split_threshold():
    from tstar_amd import jpeg
    m = jpeg.SPLIT_MIN_BYTES
    assert jpeg.split_threshold(m, m - 1) == 0 and jpeg.split_threshold(m, m) == m and jpeg.split_threshold(m, 10 * m) == m
    assert jpeg.split_threshold(0, 0) == 0 and jpeg.split_threshold(0, 1 << 20) == 0

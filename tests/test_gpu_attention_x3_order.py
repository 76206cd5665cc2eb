"""attention_x3_kernel's block order: the XCD-grouped order (the query tiles of one (image, head) back to back on one XCD, the grid
padded with blocks that exit at once) against the linear order.  Only which hardware block computes a tile changes, so the outputs
are equal bit for bit, rows behind the output included (a padding block, or a block decoded to a wrong tile, must write nothing)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [(1, 12, 577),      # 60 blocks: not a multiple of 8, four padding groups
          (3, 12, 577),      # 180 blocks
          (2, 12, 65),       # one query tile per head: groups of one block
          (1, 12, 337)]      # the masked last key tile, three query tiles
GUARD = 64


@pytest.mark.parametrize("B,heads,T", SHAPES)
def test_orders_give_the_same_bits(B, heads, T):
    from tstar_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rs = np.random.RandomState(100 + T + B)
    qkv = torch.from_numpy(rs.standard_normal((B * T, 3 * heads * 64)).astype(np.float32)).cuda()
    outs = []
    for order in (0, 1, None):                                         # None: the library's own choice (tstar_attention_x3)
        out = torch.full((B * T + GUARD, heads * 64), -7.0, dtype=torch.float32, device="cuda")
        if order is None:
            _lib.check(lib.tstar_attention_x3(qkv.data_ptr(), out.data_ptr(), B, T, heads, st), "tstar_attention_x3")
        else:
            _lib.check(lib.tstar_attention_x3_order(qkv.data_ptr(), out.data_ptr(), B, T, heads, order, st), "tstar_attention_x3_order")
        torch.cuda.synchronize()
        assert bool((out[B * T:] == -7.0).all()), f"order {order} wrote behind the output"
        outs.append(out[:B * T].view(torch.int32).cpu().numpy())
    assert np.isfinite(outs[0].view(np.float32)).all() and not (outs[0].view(np.float32) == -7.0).any()
    assert np.array_equal(outs[0], outs[1]), "the XCD-grouped order changed output bits"
    assert np.array_equal(outs[0], outs[2])


def test_order_argument_is_checked():
    from tstar_amd import _lib
    lib = _lib.load()
    x = torch.zeros((65, 3 * 64), device="cuda")
    o = torch.zeros((65, 64), device="cuda")
    assert lib.tstar_attention_x3_order(x.data_ptr(), o.data_ptr(), 1, 65, 1, 2, None) == 1 and b"order" in lib.tstar_last_error()
    assert lib.tstar_attention_x3_order(None, o.data_ptr(), 1, 65, 1, 1, None) == 1

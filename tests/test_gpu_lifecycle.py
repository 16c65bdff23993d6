"""A receiver handle's life -- create, two short pushes, flush, close -- through every configuration that allocates, or creates a stream or
an event, on a path of its own (mcrx_hip.hip: create_tables / create_buffers / create_streams_and_events, and the late allocations of
the direct path, the monitor and the K = 7 decoder), twelve times over in one process: the frames are those of the default receiver on
the same traffic, and the device memory that is free afterwards says that mcrx_hip_destroy gave everything back.

All receivers are small (M = 64, cp = 16, taper = 4, max_payload_len = 64, batch_samples = 4096; N = 2, the front ends at N = 4, the
single synchronizer at N = 1).  The traffic is made on the GPU once: two frames per channel, quantised to sc16 so that the sc16 receiver
and the cf32 ones (on the dequantised floats: the same numbers, include/mcrx_hip.h) take the same samples.  A receiver's frames are
compared as (channel, header, payload, payload_valid); the single synchronizer has no default receiver of its own shape to be compared
with (its traffic is channel-rate samples), so its frames are held to what was sent, as everybody's are."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, CP, TAPER, PAYLOAD = 64, 16, 4, 64
CFG = dict(max_payload_len=PAYLOAD, batch_samples=4096)
ROUNDS = 12


def key(frames):
    return sorted((f.channel, f.header, f.payload, f.payload_valid) for f in frames)


def sent_key(sent):
    return sorted((c, h, p, 1) for c, fr in enumerate(sent) for h, p in fr)


class Traffic(object):
    """two frames per channel of an N-channel transmitter, as sc16 words and as the floats they mean; device resident"""

    def __init__(self, product, N, fec1):
        import torch
        tx = product.multichanneltx(N, M, CP, TAPER, max_payload_len=PAYLOAD)
        iq, self.sent = tx.generate(2, PAYLOAD, fec1=fec1, seed=7 + N)
        tx.close()
        x = torch.view_as_real(iq).reshape(-1)
        self.q = torch.round(x * (0.45 * 32768.0 / float(x.abs().max()))).to(torch.int16)          # peak 0.45 of full scale
        self.x = torch.view_as_complex((self.q.to(torch.float32) * 2.0 ** -15).reshape(-1, 2)).contiguous()
        self.N, self.half = N, len(self.x) // (2 * 32 * N) * (32 * N)                                # the cut between the two pushes: whole tiles


def receive(product, t, monitor=False, host=False, **cfg):
    """create, push, flush, close -> the frames' key"""
    import torch
    kw = dict(CFG); kw.update(cfg)
    rx = product.multichannelrx(t.N, M, CP, TAPER, **kw)
    if monitor:
        rx.monitor_enable(64, "hann")
    if host:                                                    # one Execute from host memory, long enough for execute_direct
        assert len(t.x) >= 64 * product.TILE * 2 * t.N
        rx.Execute(t.x.cpu().numpy())
    else:
        s = t.q if kw.get("input_format") == "sc16" else t.x
        cut = 2 * t.half if s is t.q else t.half
        rx.Execute(s[:cut])
        torch.cuda.synchronize()                                # (what the first push reported -- a frame with the K = 7 code -- is there for the second)
        rx.Execute(s[cut:])
    rx.Flush()
    if monitor:
        r = rx.monitor_read()
        assert r.nsamp > 0 and np.all(r.level > 0)
    k = key(rx.frames)
    rx.close()
    return k


def single_synchronizer(product):
    """one frame generator -> one synchronizer, no channelizer (N = 1, single_channel): two pushes of channel-rate samples"""
    fg = product.ofdmflexframegen(M, CP, TAPER)
    sent = [(bytes(range(8)), bytes(range(PAYLOAD))), (bytes(range(8, 16)), bytes(range(1, PAYLOAD + 1)))]
    x = np.concatenate([fg.frame(h, p) for h, p in sent] + [np.zeros(4 * (M + CP), np.complex64)])
    fg.close()
    x = np.concatenate([x, np.zeros((-len(x)) % product.TILE, np.complex64)])
    rx = product.ofdmflexframesync(M, CP, TAPER, **CFG)
    half = len(x) // 2 // product.TILE * product.TILE
    rx.execute(x[:half]); rx.execute(x[half:])
    rx.Flush()
    k = key(rx.frames)
    rx.close()
    assert k == sent_key([sent])


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def footprint(product):
    """device memory a default handle of this size holds while it is alive"""
    before = free_bytes()
    rx = product.multichannelrx(2, M, CP, TAPER, **CFG)
    alive = free_bytes()
    rx.close()
    assert before > alive
    return before - alive


def test_every_kind_of_handle_lives_and_dies_twelve_times_without_a_leak(product):
    t2, t4 = Traffic(product, 2, product.LIQUID_FEC_HAMMING128), Traffic(product, 4, product.LIQUID_FEC_HAMMING128)
    k7 = Traffic(product, 2, product.LIQUID_FEC_CONV_V27)
    one = footprint(product)
    want2, want4, want7 = receive(product, t2), receive(product, t4), receive(product, k7)
    assert want2 == sent_key(t2.sent) and want4 == sent_key(t4.sent) and want7 == sent_key(k7.sent)
    free_after = {}
    for rnd in range(1, ROUNDS + 1):
        assert receive(product, t2) == want2                                        # the default receiver
        assert receive(product, t2, serial=1) == want2
        single_synchronizer(product)
        assert receive(product, t4, front_end=1) == want4
        assert receive(product, t4, front_end=2) == want4
        assert receive(product, t2, input_format="sc16") == want2
        assert receive(product, t2, scout_build=2) == want2
        assert receive(product, t2, acquisition=4) == want2
        assert receive(product, t2, monitor=True) == want2
        assert receive(product, t2, host=True) == want2                             # the direct path: its stream, events and two buffers
        assert receive(product, k7, conv_scratch=0) == want7                        # the K = 7 decoder's scratch, allocated behind the first push
        free_after[rnd] = free_bytes()
    # A handle that leaked a tenth of itself per round would be ten tenths down by round 12; the allocator's granularity is not.
    lost = free_after[2] - free_after[ROUNDS]
    print("footprint %.1f MB, free after round 2 %.1f MB, after round %d %.1f MB: %.1f MB less" %
          (one / 1e6, free_after[2] / 1e6, ROUNDS, free_after[ROUNDS] / 1e6, lost / 1e6))
    assert lost < one, (lost, one)


@pytest.mark.parametrize("bad", [dict(front_end=3), dict(conv_scratch=3)])
def test_a_configuration_refused_late_allocates_nothing(product, bad):
    one = footprint(product)
    before = free_bytes()
    with pytest.raises(ValueError):
        product.multichannelrx(2, M, CP, TAPER, **dict(CFG, **bad))
    assert abs(before - free_bytes()) < one

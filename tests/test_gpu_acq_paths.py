"""The launch paths of the receiver's host side that only appear after several pushes (mcrx_hip.hip: launch_sync and its parts, driven
by csrc/acq_plan.hpp), each held to the oracle: bytes exactly, equalised symbols to 1e-5 (test_gpu_parity.check_frames).
One small stream per code -- 4 channels, M = 64, cp = 8, QPSK, payloads of 100 bytes, 40 frames per channel, cut into 14 pushes so that
the side stream comes in (from the eighth launch on) and the cadence detector's window of 8 launches turns over -- and its oracle
frames are computed once and shared."""
import pytest

pytestmark = pytest.mark.gpu

N, M, CP, TAPER, PLEN, FRAMES, PUSHES = 4, 64, 8, 4, 100, 40, 14
_streams = {}


def _stream(oracle, product, fec1):
    """(the stream as a CUDA tensor, the oracle's frames on it), cached per code"""
    if fec1 not in _streams:
        tx = product.multichanneltx(N, M, CP, TAPER)
        iq, _ = tx.generate(FRAMES, PLEN, mod=product.LIQUID_MODEM_QPSK, fec1=fec1, seed=4100 + fec1)
        tx.close()
        iq = iq[:int(iq.numel()) // (32 * N) * (32 * N)]
        ora = oracle.MultiChannelRx(N, M, CP, TAPER)
        ora.execute(iq.cpu().numpy())
        assert len(ora.frames) == N * FRAMES and all(f.payload_valid for f in ora.frames)
        _streams[fec1] = (iq, ora.frames)
    return _streams[fec1]


def _pushes(iq, count, unit):
    """cut into `count` pushes of whole tiles (the last one takes the rest)"""
    n = int(iq.numel())
    step = (n // count + unit - 1) // unit * unit
    cuts = [iq[i:min(i + step, n)] for i in range(0, n, step)]
    assert len(cuts) >= count - 1 and len(cuts) >= 12
    return cuts


def _receive(product, cuts, **cfg):
    from test_gpu_parity import check_frames
    rx = product.multichannelrx(N, M, CP, TAPER, max_payload_len=128, **cfg)
    for x in cuts:
        rx.Execute(x)
    rx.Flush()
    frames, stats = list(rx.frames), rx.spec_stats()
    rx.close()
    return frames, stats, check_frames


@pytest.mark.parametrize("acquisition,fec1", [(0, 6), (1, 6), (2, 6), (3, 6), (5, 6), (0, 11)])
def test_every_acquisition_mode_over_many_pushes(oracle, product, acquisition, fec1):
    """acquisition = 0 (the host's choice), 1 (one launch of segment waves), 2 (the scouts walk), 3 (the anchor phase, always), 5 (a cadence
    taken for granted) on Hamming(12,8) frames; and the K = 7 code, whose frames bring the decoder's scratch (allocated by the launch after
    the device reports the code) and the general decoder's launch on the side stream."""
    iq, want = _stream(oracle, product, fec1)
    frames, (walked, adopted), check_frames = _receive(product, _pushes(iq, PUSHES, 32 * N), acquisition=acquisition)
    check_frames(frames, want)
    if acquisition == 2:
        assert adopted == 0, (walked, adopted)          # no segment waves: nothing to adopt
    else:
        assert adopted > 0, (walked, adopted)


def test_slots_grow_for_a_push_of_hundreds_of_frames(oracle, product):
    """Two channels: two pushes of 12 frames per channel, then one of 300 -- more than its segment waves' share of the 256 slots per
    channel holds, so the slot array grows in the middle of the stream (mcrx_hip.hip: sync_lazy_allocs) -- then 12 again."""
    import torch
    from test_gpu_parity import check_frames
    n2 = 2
    tx = product.multichanneltx(n2, M, CP, TAPER)
    slabs = [tx.generate(nf, PLEN, seed=4300 + i)[0] for i, nf in enumerate((12, 12, 300, 12))]
    tx.close()
    slabs = [x[:int(x.numel()) // (32 * n2) * (32 * n2)] for x in slabs]
    ora = oracle.MultiChannelRx(n2, M, CP, TAPER)
    ora.execute(torch.cat(slabs).cpu().numpy())
    assert len(ora.frames) == n2 * 336
    rx = product.multichannelrx(n2, M, CP, TAPER, max_payload_len=128, max_frames=n2 * 336 + 64)
    for x in slabs:
        rx.Execute(x)
        torch.cuda.synchronize()            # (the frame counts that size the next push's slots reach the host)
    rx.Flush()
    walked, adopted = rx.spec_stats()
    check_frames(rx.frames, ora.frames)
    # the long push holds 300 of the 336 frames of a channel: walked instead of acquired by segment waves, it would leave 11 % adopted at most
    assert adopted >= 0.5 * (walked + adopted), (walked, adopted)
    rx.close()


def test_config_struct_that_ends_behind_batch_samples(oracle, product):
    """A caller whose mcrx_hip_config ends behind batch_samples: the fields in front are honoured, whatever the memory behind holds is
    not -- acquisition = 4 (no speculation), skip_framesyms, serial and an out-of-range worker_build there change nothing."""
    iq, want = _stream(oracle, product, 6)
    frames, (walked, adopted), check_frames = _receive(product, _pushes(iq, PUSHES, 32 * N), struct_size=product.Config.single_channel.offset,
                                                       acquisition=4, skip_framesyms=1, serial=1, worker_build=9)
    check_frames(frames, want)              # (the symbols are there: skip_framesyms was not read)
    assert all(len(f.framesyms) for f in frames)
    assert adopted > 0, (walked, adopted)   # (segment waves ran: acquisition = 4 was not read)

"""A device-side delay on a chosen stream, for tests that need work on that stream to still be pending while the host goes on
(tests/test_jpeg_streams.py).

stall(stream, seconds) enqueues the delay on `stream`, records an event right after it and returns that event: while
event.query() is False, everything enqueued on `stream` after the stall has not started.  The delay is torch.cuda._sleep, whose
cycle count is calibrated once per process: a short sleep is timed with events on a stream and scaled (the counter it reads may
tick at the shader clock or at a fixed 100 MHz).  Without that attribute the delay is a chain of large device-to-device copies,
calibrated the same way.  The returned event carries .started (the event recorded in front of the delay) and .seconds (what was
asked for), so that a test can assert afterwards, from the device's own clock, that the stall was as long
as it was meant to be (measured_seconds)."""
import torch

PROBE_CYCLES = 100_000  # the first calibration sleep: 1 ms if the counter ticks at 100 MHz, 0.05 ms at a 2 GHz shader clock
COPY_BYTES = 256 << 20  # one link of the copy chain: ~0.1 ms at HBM speed

_rate = None  # cycles per second of _sleep, or copies per second of the chain
_copy_buffers = None


def _delay(units):
    """the delay on the current stream: `units` sleep cycles, or copies of the chain"""
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(units))
    else:
        a, b = _copy_buffers
        for _ in range(int(units)):
            b.copy_(a, non_blocking=True)


def calibrate(stream=None):
    """-> units of delay per second; measured once (two probes, the second after the clocks have come up) and kept"""
    global _rate, _copy_buffers
    if _rate is not None:
        return _rate
    use_sleep = hasattr(torch.cuda, "_sleep")
    if not use_sleep:
        _copy_buffers = (torch.zeros(COPY_BYTES, dtype=torch.uint8, device="cuda"), torch.empty(COPY_BYTES, dtype=torch.uint8, device="cuda"))
    probe = PROBE_CYCLES if use_sleep else 4
    s = torch.cuda.Stream() if stream is None else stream
    ms = 0.0
    for _ in range(8):  # the counter _sleep reads may tick at the shader clock or at a fixed 100 MHz: grow the probe until it takes 2 ms
        for _ in range(2):  # the second after the clocks have come up
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                a.record()
                _delay(probe)
                b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
        if ms >= 2.0:
            break
        probe *= 8
    assert ms >= 2.0, f"the calibration delay of {probe} units took {ms} ms: no delay to scale"
    _rate = probe / (ms * 1e-3)
    return _rate


def stall(stream, seconds):
    """enqueue a delay of `seconds` on `stream`; -> the event recorded right after it (.started: the event in front, .seconds)"""
    rate = calibrate()
    start, done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        start.record()
        _delay(max(1, round(seconds * rate)))
        done.record()
    done.started, done.seconds = start, seconds
    return done


def measured_seconds(event):
    """how long the stall that returned `event` took on the device; call after the event has completed"""
    return event.started.elapsed_time(event) * 1e-3

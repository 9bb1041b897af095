"""Device buffers of the GPU tests of the list and keyed-sequence operations
(tests/test_gpu_{reduce,scan,filter,table,top,rollup}.py): an array's bytes on the device at a chosen
alignment, a buffer's address, and a batch of calls on the current stream."""
import numpy as np


def up(a, skew=0):
    """a's bytes on the device (uint8); skew: that many bytes past a 256-byte boundary"""
    import torch
    a = np.ascontiguousarray(a).view(np.uint8)
    buf = torch.zeros(len(a) + 256, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 256 == 0
    buf[skew:skew + len(a)] = torch.from_numpy(a)
    return buf[skew:skew + len(a)]


def ptr(t):
    """a buffer's address, NULL for one of no byte"""
    return t.data_ptr() if t.numel() else None


def run(gpu, devs):
    """enqueue every call of devs on the current stream, then wait for them all"""
    import torch
    for d in devs:
        assert d.enqueue(gpu, torch.cuda.current_stream()) == 0
    torch.cuda.synchronize()

"""Between a caller's tensors and the C ABI: the one tensor check, the one pointer and the one way to open a call's outputs that every
entry point on device memory (gnxraytracer_amd/__init__.py) is written with -- the Python side of csrc/api_device_call.hip.h.  Nothing
here loads the library or touches a GPU before a check has passed; torch is imported where a tensor is looked at."""
import ctypes as C

import numpy as np

ANY_GPU = "a GPU"   # `device` of the checks: a tensor on whichever GPU (the message prints it as it stands)
SOME = "at least one"   # a dimension of a shape pattern that must not be empty


def _got(x, type_name=True, device=True):
    """The tail of every refusal: what the caller handed in.  The only place that reads type, dtype, shape and device of an object that
    may be anything; the flags keep the messages that leave the type name or the device out as they are."""
    return (f"{type(x).__name__} " if type_name else "") + f"{getattr(x, 'dtype', None)} {tuple(getattr(x, 'shape', ()))}" + (f" on {getattr(x, 'device', None)}" if device else "")


def _is_torch(x):
    """an object of torch's, told without importing torch (the host-memory paths never do)"""
    return type(x).__module__.split(".")[0] == "torch"


def _fits(shape, pattern):
    """`pattern`: per dimension a size, None (any) or SOME"""
    if len(shape) != len(pattern):
        return False
    for have, want in zip(shape, pattern):
        if want is not None and (have < 1 if want is SOME else have != want):
            return False
    return True


def _is_tensor(x, dtype, pattern, device=None):
    """The predicate of every check: a contiguous torch tensor of `dtype` whose shape fits `pattern`, and `device`: None (layout only),
    ANY_GPU, an int (a GPU by its index: a scene's device) or a torch.device (equal to it: the device of the call's first array)."""
    import torch
    if not (isinstance(x, torch.Tensor) and x.dtype == dtype and _fits(x.shape, pattern) and x.is_contiguous()):
        return False
    if device is None:
        return True
    if device is ANY_GPU or isinstance(device, int):
        return x.is_cuda and (device is ANY_GPU or x.device.index == device)
    return x.device == device


def _refuse(x, phrase, type_name=True, device=True):
    """The refusal of every check (`if not _is_tensor(...): _refuse(...)`, so that a message is only put together when it is needed):
    `phrase` is the call's own wording up to ", got"."""
    raise ValueError(f"{phrase}, got {_got(x, type_name, device)}")


def _expect(what, x, dtype, tail, device=None):
    """`x` is a contiguous `dtype` tensor (n, *tail), in the wording "<what>: expected a contiguous torch.float32 (n, 8) tensor on cuda:0";
    device=None checks the layout alone and names no device."""
    if not _is_tensor(x, dtype, (None, *tail), device):
        where = "" if device is None else f" on {'cuda:%d' % device if isinstance(device, int) else device}"
        _refuse(x, f"{what}: expected a contiguous {dtype} (n{''.join(', %d' % c for c in tail)}) tensor{where}", device=device is not None)
    return x


def _image_size(name, width, height, noun="image"):
    width, height = int(width), int(height)
    if width <= 0 or height <= 0:
        raise ValueError(f"{name}: invalid {noun} size {width} x {height}")
    return width, height


def _image(name, arg, x, size=True):
    """`x` is an image of the calls without a scene, (H, W, 4) or (V, H, W, 4) float32 on a GPU: (shape, V, H, W).  size=False leaves the
    refusal of an empty image to the caller, who has other arguments to refuse first."""
    import torch
    if not (_is_tensor(x, torch.float32, (None, None, 4), ANY_GPU) or _is_tensor(x, torch.float32, (None, None, None, 4), ANY_GPU)):
        _refuse(x, f"{name}: {arg} must be a contiguous float32 (H, W, 4) or (V, H, W, 4) tensor on a GPU")
    shape = tuple(x.shape)
    if size:
        _image_size(name, shape[-2], shape[-3])
    return shape, (shape[0] if len(shape) == 4 else 1), shape[-3], shape[-2]


def _same_count(name, what, k, n, first, noun="rows"):
    """`what` has k rows / entries for the n of the call's first array (what=None: "<k> <noun> for <n> <first>")"""
    if k != n:
        raise ValueError(f"{name}: {what + ' has ' if what else ''}{k} {noun} for {n} {first}")


def _only_kw(name, kw, allowed):
    unknown = [k for k in kw if k not in allowed]
    if unknown:
        raise ValueError(f"{name}: unexpected arguments {unknown} ({', '.join(allowed)})")


def _ptr(x):
    """a tensor's address for the C ABI (None stays None, an empty tensor is a null pointer)"""
    return None if x is None else C.c_void_p(x.data_ptr() or None)


def _addr(a):
    """an address or a hipStream_t held as an int (0: null)"""
    return C.c_void_p(a or None)


def _stream_handle(what, stream):
    """`stream` of the scene-editing calls -- None (the null stream), a torch.cuda.Stream or a hipStream_t as an integer -- as an int;
    TypeError for anything else, ValueError for a negative handle, both before the library is reached."""
    import numbers
    if stream is None:
        return 0
    if isinstance(stream, numbers.Integral) and not isinstance(stream, bool):
        handle = int(stream)
    elif isinstance(getattr(stream, "cuda_stream", None), int):
        handle = stream.cuda_stream   # a torch.cuda.Stream
    else:
        raise TypeError(f"{what}: stream must be None, a torch.cuda.Stream or a hipStream_t as an integer, got {type(stream).__name__}")
    if handle < 0:
        raise ValueError(f"{what}: a hipStream_t is not negative, got {handle}")
    return handle


def _stream_pair(stream, device):
    """`stream` -- None (torch's current stream on `device`), a torch.cuda.Stream, or a hipStream_t as an int -- as the pair
    (hipStream_t as an int, torch stream of that handle)."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream(device)
    elif isinstance(stream, int):
        stream = torch.cuda.ExternalStream(stream, device=device)
    return stream.cuda_stream, stream


def _out_tensor(what, out, shape, dtype, device):
    """The result tensor of a call on device memory: `out` when given -- it must be a contiguous `dtype` tensor of `shape` on `device`,
    the device of the call's inputs or of its scene -- else a new one."""
    import torch
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not _is_tensor(out, dtype, shape, device):
        _refuse(out, f"{what} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}")
    return out


def _outputs(stream, device, *results):
    """Opens the outputs of a call: `results` are (what, given or None, shape, dtype) each.  Returns (hipStream_t as an int, torch stream,
    one tensor per result), the new ones allocated under that stream."""
    import torch
    hstream, tstream = _stream_pair(stream, device)
    with torch.cuda.stream(tstream):   # (the caching allocator ties the new tensors to the stream that writes them)
        return (hstream, tstream) + tuple(_out_tensor(what, out, shape, dtype, device) for what, out, shape, dtype in results)


def _host_or_device(prefix, x, dtype, patterns, text, device, on_device=None, tensor_text=None, or_none=False):
    """An array of a scene-editing method: a numpy array in host memory or a contiguous torch tensor on the scene's device, of numpy dtype
    `dtype` and a shape that fits one of `patterns`.  Returns (address, the object to keep alive -- the contiguous array or the tensor --,
    on_device).  on_device=None: the array alone decides, and its messages name no type; True / False: the call takes several arrays,
    all tensors or all numpy, and says so.  `text`: the shape as the messages print it; `tensor_text`: the tensor's words where they are not
    "<text> tensor"."""
    kind = np.dtype(dtype).name
    together = on_device is not None
    there, here = (" (all arrays tensors there, or all numpy)", " in host memory (all arrays numpy, or all tensors on the scene's device)") if together else ("", "")
    if on_device is None:
        on_device = not isinstance(x, np.ndarray)
        if on_device and not _is_torch(x):
            raise ValueError(f"{prefix}: expected a numpy array{', a torch tensor or None' if or_none else ' or a torch tensor'}, got {type(x).__name__}")
    if on_device:
        import torch
        if not any(_is_tensor(x, getattr(torch, kind), p, device) for p in patterns):
            _refuse(x, f"{prefix}: expected a contiguous {kind} {tensor_text or text + ' tensor'} on cuda:{device}{there}", type_name=together)
        return x.data_ptr(), x, True
    if not (isinstance(x, np.ndarray) and x.dtype == dtype and any(_fits(x.shape, p) for p in patterns)):
        _refuse(x, f"{prefix}: expected {'an' if kind[0] == 'i' and not together else 'a'} {kind} array of shape {text}{here}", type_name=together, device=False)
    x = np.ascontiguousarray(x)
    return x.ctypes.data, x, False


def _arrays_on_device(name, what, first):
    """The rule of the editing calls that take several arrays -- all numpy, or all tensors on the scene's device --, decided by the first."""
    if isinstance(first, np.ndarray):
        return False
    if not _is_torch(first):
        raise ValueError(f"{name}: {what}: expected a numpy array or a torch tensor, got {type(first).__name__}")
    return True


def _edit_stream(stream, x):
    """`stream` of an editing call defaults to torch's current stream when the data is a tensor on a GPU"""
    if stream is None and _is_torch(x) and getattr(x, "is_cuda", False):
        import torch
        return torch.cuda.current_stream(x.device)
    return stream

"""Device allocations, copies and streams for the GPU tests that hand the library device pointers of their own, through the HIP
runtime libvio_amd.so is linked against."""
import ctypes as C


class Hip:
    def __init__(self):
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        hip.hipStreamDestroy.argtypes = [C.c_void_p]
        self.hip = hip

    def upload(self, a):
        d = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(d), a.nbytes) == 0 and self.hip.hipMemcpy(d, a.ctypes.data, a.nbytes, 1) == 0
        return d

    def download(self, d, a):
        assert self.hip.hipMemcpy(a.ctypes.data, d, a.nbytes, 2) == 0
        return a

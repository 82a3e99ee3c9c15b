"""Child process of tests/test_volume.py (case 9): runs raw audio files through the STOCK `volume` element with a linear
GstInterpolationControlSource bound to its `volume` property - the CPU reference the numpy model is checked against.  Loads
libgstreamer-1.0 / libgstcontroller-1.0 with ctypes; touches neither the product library nor a GPU.

usage: volume_stock_child.py jobs.json     { "lib": dir, "jobs": [ { src, dst, pcm, channels, frames, rate, c0, c1 }, ... ] }
c0 / c1: the control values (0 .. 1 maps to the property's 0 .. 10) at the first frame and at the end of the file."""
import ctypes as C
import json
import os
import sys

GST_SECOND = 1000000000
GST_STATE_NULL, GST_STATE_PLAYING = 1, 4
GST_MESSAGE_EOS, GST_MESSAGE_ERROR = 1, 2
GST_INTERPOLATION_MODE_LINEAR = 1
MESSAGE_TYPE_OFFSET = 64        # sizeof (GstMiniObject) on LP64: GstMessage.type follows it


def main(path):
    spec = json.load(open(path))
    gobj = C.CDLL(os.path.join(spec["lib"], "libgobject-2.0.so.0"), mode=C.RTLD_GLOBAL)
    gst = C.CDLL(os.path.join(spec["lib"], "libgstreamer-1.0.so.0"), mode=C.RTLD_GLOBAL)
    ctl = C.CDLL(os.path.join(spec["lib"], "libgstcontroller-1.0.so.0"), mode=C.RTLD_GLOBAL)
    gst.gst_parse_launch.restype = C.c_void_p
    gst.gst_parse_launch.argtypes = [C.c_char_p, C.c_void_p]
    gst.gst_bin_get_by_name.restype = C.c_void_p
    gst.gst_bin_get_by_name.argtypes = [C.c_void_p, C.c_char_p]
    gst.gst_element_set_state.argtypes = [C.c_void_p, C.c_int]
    gst.gst_element_get_bus.restype = C.c_void_p
    gst.gst_element_get_bus.argtypes = [C.c_void_p]
    gst.gst_bus_timed_pop_filtered.restype = C.c_void_p
    gst.gst_bus_timed_pop_filtered.argtypes = [C.c_void_p, C.c_uint64, C.c_int]
    gst.gst_object_add_control_binding.argtypes = [C.c_void_p, C.c_void_p]
    gst.gst_object_unref.argtypes = [C.c_void_p]
    gst.gst_mini_object_unref.argtypes = [C.c_void_p]
    ctl.gst_interpolation_control_source_new.restype = C.c_void_p
    ctl.gst_timed_value_control_source_set.argtypes = [C.c_void_p, C.c_uint64, C.c_double]
    ctl.gst_direct_control_binding_new.restype = C.c_void_p
    ctl.gst_direct_control_binding_new.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    gobj.g_object_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
    gst.gst_init(None, None)
    for j in spec["jobs"]:
        size = os.path.getsize(j["src"])
        desc = ("filesrc location=%s blocksize=%d ! rawaudioparse format=pcm pcm-format=%s sample-rate=%d num-channels=%d ! volume name=vol ! "
                "filesink location=%s" % (j["src"], size, j["pcm"], j["rate"], j["channels"], j["dst"]))
        pipe = gst.gst_parse_launch(desc.encode(), None)
        if not pipe:
            sys.exit("gst_parse_launch failed: " + desc)
        vol = gst.gst_bin_get_by_name(pipe, b"vol")
        if not vol:
            sys.exit("no volume element in: " + desc)
        cs = ctl.gst_interpolation_control_source_new()
        gobj.g_object_set(cs, b"mode", GST_INTERPOLATION_MODE_LINEAR, None)
        end = j["frames"] * GST_SECOND // j["rate"]
        if not ctl.gst_timed_value_control_source_set(cs, 0, j["c0"]) or not ctl.gst_timed_value_control_source_set(cs, end, j["c1"]):
            sys.exit("gst_timed_value_control_source_set failed")
        if not gst.gst_object_add_control_binding(vol, ctl.gst_direct_control_binding_new(vol, b"volume", cs)):
            sys.exit("gst_object_add_control_binding failed")
        gst.gst_element_set_state(pipe, GST_STATE_PLAYING)
        bus = gst.gst_element_get_bus(pipe)
        msg = gst.gst_bus_timed_pop_filtered(bus, 20 * GST_SECOND, GST_MESSAGE_EOS | GST_MESSAGE_ERROR)
        kind = C.c_uint.from_address(msg + MESSAGE_TYPE_OFFSET).value if msg else 0
        if msg:
            gst.gst_mini_object_unref(msg)
        gst.gst_element_set_state(pipe, GST_STATE_NULL)
        gst.gst_object_unref(bus)
        gst.gst_object_unref(vol)
        gst.gst_object_unref(cs)
        gst.gst_object_unref(pipe)
        if kind != GST_MESSAGE_EOS:
            sys.exit("the pipeline did not reach EOS (message type %d): %s" % (kind, desc))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))

"""The reader of every progressive Huffman JPEG (SOF2) the GPU decoder takes: spectral selection and successive approximation (ITU-T
T.81 Annex G), with or without restart markers -- libjpeg's standard scan script (Pillow's progressive=True, jpegtran -progressive)
as well as what jfif.write_progressive_jpeg writes.

jfif.read_progressive_jpeg stays the reader of the engine's own files and keeps refusing successive approximation and scans without
restart markers; read_sof2_jpeg returns an equal dict for every file that one accepts.
"""
from . import jfif
from .jfif import JpegFormatError


def read_sof2_jpeg(data):
    """Parse a progressive Huffman JPEG (SOF2).  Returns jfif.read_jpeg's dict with sof = 0xC2; every scan also carries 'ss', 'se',
    'ah', 'al' (its band, zig-zag, and its successive approximation), and its 'huffman' and 'restart_interval' (0: no restart markers)
    are those in force at it.  A DC scan's components carry a 'ta' and an AC scan's a 'td' the scan does not use; a DC refinement
    scan uses neither.

    The rules for segments, frame header, DQT, DHT and the SOS header are read_jpeg's own, applied to a copy of the file whose frame
    marker is rewritten to SOF1 and whose bands to 0..63 (jfif.read_progressive_jpeg's twin file).  On top of them this refuses
    (JpegFormatError) a file that is not SOF2, an interleaved AC scan, a band that mixes DC and AC or is out of order, Al above 13, and
    what T.81 G.1.1.1.2 forbids per component and coefficient position: a first scan (Ah = 0) of a position that was coded before, a
    refinement of a position that was not, a refinement whose Ah is not the Al last coded there or whose Al is not Ah - 1, and an AC
    scan of a component whose DC first scan has not come.  A band that no scan codes is legal (those coefficients are zero), and so
    is a position whose last scan leaves Al > 0 (a truncated script: libjpeg decodes what is there)."""
    data = bytes(data)
    sof = jfif.sof_marker(data)
    if sof != 0xC2:
        if sof is None:
            jfif.read_jpeg(data, require_restart=False)  # malformed before any frame header: its message
        raise JpegFormatError(f"not a progressive file: the frame header is SOF{(sof or 0xC0) - 0xC0}, not SOF2")
    twin, bands = bytearray(data), []
    for m, p, n in jfif._segments(data):
        if m == 0xC2:
            twin[p - 3] = 0xC1
        elif m == 0xDA and n and n == 4 + 2 * data[p]:  # (any other SOS is malformed: read_jpeg says so)
            bands.append(tuple(data[p + n - 3:p + n]))
            twin[p + n - 3:p + n] = bytes([0, 63, 0])
    info = jfif.read_jpeg(bytes(twin), require_restart=False)
    info["sof"] = 0xC2
    last_al = [{} for _ in info["components"]]  # per component: zig-zag position -> the Al it was last coded with
    for k, (sc, (ss, se, a)) in enumerate(zip(info["scans"], bands)):
        ah, al = a >> 4, a & 15
        sc.update(ss=ss, se=se, ah=ah, al=al)
        if ss > se or se > 63 or (ss == 0 and se != 0):
            raise JpegFormatError(f"malformed SOS: band {ss}..{se} (scan {k}; 0..0, or an AC band inside 1..63)")
        if ss > 0 and len(sc["components"]) > 1:
            raise JpegFormatError(f"malformed SOS: an interleaved AC scan (scan {k}: T.81 G.1.1.1.1)")
        if al > 13:
            raise JpegFormatError(f"malformed SOS: successive approximation Al {al} (scan {k}; 0..13)")
        for c in sc["components"]:
            coded = last_al[c["index"]]
            if ss > 0 and 0 not in coded:
                raise JpegFormatError(f"malformed file: an AC scan of component {c['index']} before its DC scan (scan {k})")
            for pos in range(ss, se + 1):
                if ah == 0 and pos in coded:
                    raise JpegFormatError(f"malformed file: a position of component {c['index']} is coded a second time (scan {k}: band {ss}..{se})")
                if ah != 0 and pos not in coded:
                    raise JpegFormatError(f"malformed file: a refinement of a position of component {c['index']} no scan has coded (scan {k}: band {ss}..{se})")
                if ah != 0 and (coded[pos] != ah or al != ah - 1):
                    raise JpegFormatError(f"malformed file: a refinement with Ah {ah}, Al {al} of a position of component {c['index']} last coded with Al "
                                          f"{coded[pos]} (scan {k}: band {ss}..{se})")
                coded[pos] = al
    return info

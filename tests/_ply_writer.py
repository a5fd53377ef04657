"""Test helper: writes small PLY files in every form geometric_adv_amd.in_out.load_ply reads (and, for the refusal tests,
some it must not).  Used by tools/make_golden_dataset.py for tests/golden/dataset/ and by tests/test_in_out_host.py."""
import numpy as np

_NP = {'char': 'i1', 'uchar': 'u1', 'short': 'i2', 'ushort': 'u2', 'int': 'i4', 'uint': 'u4', 'float': 'f4', 'double': 'f8',
       'float32': 'f4', 'float64': 'f8'}


def _fmt(v, code):
    if code == 'f4':
        return '%.9g' % float(np.float32(v))           # nine digits round-trip a float32
    if code == 'f8':
        return '%.17g' % float(v)
    return '%d' % int(v)


def write_ply(path, elements, fmt='ascii', comments=(), obj_info=(), truncate=None):
    """elements: [(name, [(property, type, values) | (property, ('list', count type, item type), rows)])] in file order; every
    property of an element has as many values as the element has entries.  fmt: 'ascii', 'binary_little_endian' or
    'binary_big_endian' (anything else is written into the format line as it is, with a little-endian body).
    truncate: number of bytes to cut off the end of the body."""
    order = '>' if fmt == 'binary_big_endian' else '<'
    head = ['ply', 'format %s 1.0' % fmt]
    head += ['comment %s' % c for c in comments] + ['obj_info %s' % c for c in obj_info]
    for name, props in elements:
        head.append('element %s %d' % (name, len(props[0][2]) if props else 0))
        for pname, ptype, _ in props:
            head.append('property list %s %s %s' % (ptype[1], ptype[2], pname) if isinstance(ptype, tuple)
                        else 'property %s %s' % (ptype, pname))
    head.append('end_header')
    body = bytearray()
    for name, props in elements:
        for k in range(len(props[0][2]) if props else 0):
            fields = []
            for pname, ptype, values in props:
                if isinstance(ptype, tuple):
                    row = list(values[k])
                    items = [(len(row), _NP[ptype[1]])] + [(v, _NP[ptype[2]]) for v in row]
                else:
                    items = [(values[k], _NP[ptype])]
                for v, code in items:
                    if fmt == 'ascii':
                        fields.append(_fmt(v, code))
                    else:
                        body += np.array(v).astype(order + code).tobytes()
            if fmt == 'ascii':
                body += (' '.join(fields) + '\n').encode('ascii')
    if truncate:
        body = body[:len(body) - truncate]
    with open(path, 'wb') as f:
        f.write(('\n'.join(head) + '\n').encode('ascii'))
        f.write(bytes(body))


def vertex(points, ptype='float', extra_before=(), extra_between=(), extra_after=()):
    """A vertex element of points (n, 3); extra_*: [(property, type, values)] placed before x, between x and y, after z."""
    p = np.asarray(points)
    return ('vertex', list(extra_before) + [('x', ptype, p[:, 0])] + list(extra_between)
            + [('y', ptype, p[:, 1]), ('z', ptype, p[:, 2])] + list(extra_after))

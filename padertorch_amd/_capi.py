"""The C ABI as ctypes, read from the text of include/ptmi.h: regular expressions over the declarations, no C grammar.

What the header can say and how it maps (everything else raises, naming the declaration - nothing defaults to ``void*`` or ``int``):

    int / int32_t / int64_t / float / double    c_int / c_int32 / c_int64 / c_float / c_double
    ptmi_stream_t                               c_void_p
    return const char*                          c_char_p
    const S* for a structure S of ``structs``   POINTER(S)      (the call sites pass a bare Structure instance)
    every other T* / T name[n]                  c_void_p        (device pointers travel as integers; host arrays as ctypes arrays)
    (void)                                      []
"""
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_void_p, POINTER

SCALARS = {'int': c_int, 'int32_t': c_int32, 'int64_t': c_int64, 'float': c_float, 'double': c_double, 'ptmi_stream_t': c_void_p}
_STRUCT = r'typedef\s+struct\s+(\w+)\s*\{([^}]*)\}\s*\1\s*;'


def _declarations(text):
    """The header without comments, preprocessor lines and the ``extern "C" {`` ... ``}`` around its declarations."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#(?:[^\n]*\\\n)*[^\n]*', ' ', text, flags=re.M)
    text, opened = re.subn(r'\bextern\s+"C"\s*\{', ' ', text)
    for _ in range(opened):
        text = text.rstrip()
        if not text.endswith('}'):
            raise ValueError('extern "C" { is not closed by a } behind the last declaration')
        text = text[:-1]
    return text


def struct_fields(text, name):
    """``_fields_`` of ``typedef struct name { ... } name;``: members ``T a;``, ``T a, b;`` and ``T a[n];`` of scalar type."""
    body = {m.group(1): m.group(2) for m in re.finditer(_STRUCT, _declarations(text))}.get(name)
    if body is None:
        raise ValueError(f'{name}: the header has no "typedef struct {name} {{...}} {name};"')
    fields = []
    for decl in filter(None, (' '.join(d.split()) for d in body.split(';'))):
        m = re.fullmatch(r'(\w+) (.+)', decl)
        if not m or m.group(1) not in SCALARS:
            raise ValueError(f'{name}: cannot map the member "{decl}"')
        for item in m.group(2).split(','):
            member = re.fullmatch(r'\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*', item)
            if not member:
                raise ValueError(f'{name}: cannot map the member "{decl}"')
            ctype = SCALARS[m.group(1)]
            fields.append((member.group(1), ctype * int(member.group(2)) if member.group(2) else ctype))
    return fields


def _squeeze(ctext):
    """``const`` dropped, one blank between words, none around ``*``: ``const uint16_t* const* b`` -> ``uint16_t**b``."""
    return re.sub(r'\s*\*\s*', '*', ' '.join(re.sub(r'\bconst\b', ' ', ctext).split()))


def _argtype(name, param, structs):
    m = re.fullmatch(r'(\w+)(\*+| )\w+(\[\w*\])?', _squeeze(param))     # type, stars, identifier, array
    if not m:
        raise ValueError(f'{name}: cannot read the parameter "{" ".join(param.split())}"')
    base, stars = m.group(1), m.group(2).strip() + ('*' if m.group(3) else '')
    if not stars:
        if base not in SCALARS:
            raise ValueError(f'{name}: no ctypes mapping for the by-value parameter type "{base}"')
        return SCALARS[base]
    return POINTER(structs[base]) if stars == '*' and base in structs else c_void_p


def signatures(text, structs):
    """``name -> (restype, argtypes)`` of every ``ptmi_*`` prototype; ``structs`` maps a structure's C name to its class."""
    text = re.sub(_STRUCT + r'|\btypedef\b[^;{]*;', ' ', _declarations(text))
    table = {}
    for decl in filter(None, (' '.join(d.split()) for d in text.split(';'))):
        m = re.fullmatch(r'(.+?)\b(ptmi_[a-z0-9_]+) ?\((.*)\)', decl)
        if not m:
            raise ValueError(f'cannot split the declaration "{decl}" into "type ptmi_name(parameters)"')
        res, name, params = _squeeze(m.group(1)), m.group(2), m.group(3).strip()
        if '(' in params:
            raise ValueError(f'{name}: function-pointer parameters have no mapping')
        if res != 'char*' and res not in SCALARS:
            raise ValueError(f'{name}: no ctypes mapping for the return type "{m.group(1).strip()}"')
        if name in table:
            raise ValueError(f'{name}: declared twice')
        table[name] = (c_char_p if res == 'char*' else SCALARS[res],
                       [] if params == 'void' else [_argtype(name, p, structs) for p in params.split(',')])
    return table

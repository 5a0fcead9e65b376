# -*- coding:utf-8 -*-
"""keras.regularizers.L1L2 / L1 / L2 as plain coefficient holders.

The value is Keras' `L1L2.__call__`: l1 * sum|x| + l2 * sum x^2.  The arithmetic runs in csrc/regularizer.hip
(ops.regularization_penalty); these classes only carry and (de)serialise the two coefficients.  Anything that is not an
L1/L2 penalty — a custom callable, 'orthogonal_regularizer', an unknown string — raises: nothing is dropped silently."""
import numbers


class Regularizer:
    l1 = 0.0
    l2 = 0.0

    def coefficients(self):
        return float(self.l1), float(self.l2)

    def __eq__(self, other):
        return isinstance(other, Regularizer) and self.coefficients() == other.coefficients()

    def __hash__(self):
        return hash(self.coefficients())

    def __repr__(self):
        return f'{type(self).__name__}({self.get_config()})'


def _coefficient(name, value):
    if value is None:
        return 0.0
    if isinstance(value, bool) or not isinstance(value, numbers.Real):
        raise ValueError(f'regularizer coefficient {name}={value!r}: expected a number')
    value = float(value)
    if value != value or value in (float('inf'), float('-inf')):
        raise ValueError(f'regularizer coefficient {name}={value!r}: expected a finite number')
    return value


class L1L2(Regularizer):
    def __init__(self, l1=0.0, l2=0.0):
        self.l1 = _coefficient('l1', l1)
        self.l2 = _coefficient('l2', l2)

    def get_config(self):
        return {'l1': self.l1, 'l2': self.l2}


class L1(Regularizer):
    def __init__(self, l1=0.01):
        self.l1 = _coefficient('l1', l1)

    def get_config(self):
        return {'l1': self.l1}


class L2(Regularizer):
    def __init__(self, l2=0.01):
        self.l2 = _coefficient('l2', l2)

    def get_config(self):
        return {'l2': self.l2}


_CLASSES = {'L1': L1, 'L2': L2, 'L1L2': L1L2}
_STRINGS = {'l1': lambda: L1(0.01), 'l2': lambda: L2(0.01), 'l1_l2': lambda: L1L2(0.01, 0.01)}


def get(identifier, knob='regularizer'):
    """None | 'l1' | 'l2' | 'l1_l2' | {'class_name': ..., 'config': ...} | L1 / L2 / L1L2 | any object with numeric `l1` and / or
    `l2` attributes (a real Keras regularizer) -> a Regularizer or None.  `knob` names the argument in the error."""
    if identifier is None:
        return None
    if isinstance(identifier, Regularizer):
        return identifier
    if isinstance(identifier, str):
        if identifier in _STRINGS:
            return _STRINGS[identifier]()
        raise ValueError(f'{knob}={identifier!r}: only the L1 / L2 penalties are supported '
                         f'({sorted(_STRINGS)}, L1 / L2 / L1L2 instances or their serialised dicts)')
    if isinstance(identifier, dict):
        name, config = identifier.get('class_name'), identifier.get('config', {})
        if name not in _CLASSES or not isinstance(config, dict):
            raise ValueError(f'{knob}={identifier!r}: class_name must be one of {sorted(_CLASSES)} with a config dict')
        try:
            return _CLASSES[name](**config)
        except (TypeError, ValueError) as e:
            raise ValueError(f'{knob}={identifier!r}: {e}') from None
    if type(identifier).__name__ == 'OrthogonalRegularizer':
        raise ValueError(f'{knob}={identifier!r}: OrthogonalRegularizer is not supported, only the L1 / L2 penalties')
    l1, l2 = getattr(identifier, 'l1', None), getattr(identifier, 'l2', None)
    if l1 is None and l2 is None:
        raise ValueError(f'{knob}={identifier!r}: only the L1 / L2 penalties are supported; a custom callable is not')
    try:
        return L1L2(None if l1 is None else float(l1), None if l2 is None else float(l2))
    except (TypeError, ValueError):
        raise ValueError(f'{knob}={identifier!r}: its l1 / l2 attributes are not numbers') from None


def serialize(reg):
    """-> the Keras serialised dict ({'class_name', 'config'}), or None"""
    if reg is None:
        return None
    reg = get(reg)
    return {'class_name': type(reg).__name__, 'config': reg.get_config()}


def active(reg):
    """the regularizer if it penalises anything (a coefficient that is not zero), else None"""
    return reg if reg is not None and (reg.l1 != 0.0 or reg.l2 != 0.0) else None

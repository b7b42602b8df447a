"""What a ``Network`` keeps from frame to frame: the rule tensors are recognised by (_resident / _still_resident) and
the one kind of entry (Kept) that asks it, for the weights an entry was built from and for the frame's inputs."""
import weakref


def _resident(tensors):
    """What _still_resident recognises ``tensors`` by later: a weak reference, the ``data_ptr`` and the ``_version`` of
    each.  THE rule of everything a Network keeps from frame to frame, for the frame's inputs (priors, bbox,
    dst_posevec) and for the parameters alike:

    * the weak reference is the identity: another object never matches, not even one that the allocator placed on the
      freed address of the old one with an equal version counter (a replaced nn.Parameter), and a collected object can
      never match again;
    * ``data_ptr`` sees ``t.data = other`` and a move between devices, which leave object and counter alone;
    * ``_version`` sees every in-place write autograd knows of: ``t.copy_()``, ``t.mul_()``, foreach ops on the
      tensors themselves, torch's optimizers in their foreach and single-tensor forms, GroupedAdam.

    What none of the three sees is a write through ``t.data`` / ``t.detach()`` (``p.data.copy_()``,
    ``p.data[i] = v``, ``dist.broadcast(p.data)``, optimizers that update through detached views): for the parameters
    that is Network.weights_changed(), which load_state_dict and a move of the module call themselves and whose effect
    a train-path forward has (Network._weights_gen); for a frame's inputs the rule is to pass a fresh tensor, or to
    write the tensor itself."""
    return tuple((weakref.ref(t), t.data_ptr(), t._version) for t in tensors)


def _still_resident(refs, tensors):
    """True when ``tensors`` are the very objects ``refs`` = _resident(...) was built from, on the same memory and
    unwritten since: a driver that keeps its per-subject tensors on the device hits without a look at their values,
    i.e. without a host synchronisation.  Equal values in other objects do not count: the caller compares those once,
    or not at all."""
    return refs is not None and len(refs) == len(tensors) \
        and all(r() is t and ptr == t.data_ptr() and v == t._version for (r, ptr, v), t in zip(refs, tensors))


class Kept:
    """One thing a Network keeps between frames.  ``key``: the plain values it depends on (mode, head, resolution);
    ``gen``: Network._weights_gen when it was built; ``weights`` / ``inputs``: _resident(the parameters it was built
    from) / _resident(the frame's tensors it was built for), None = none remembered; ``injected``: given from outside,
    not derived from the weights -- Network.weights_changed() leaves it.  The rest is payload, None where an entry has
    none: ``packed`` + ``serial`` (a canonical image and the number of its pack), ``vol`` + ``priors`` (the weight
    volume), ``grid`` + ``bmin`` + ``bmax`` (a baked grid over its box), ``nr_packed`` (the non-rigid image an offset
    grid was baked on), ``value`` (a head id read back)."""
    _PAYLOAD = ('packed', 'serial', 'vol', 'priors', 'grid', 'bmin', 'bmax', 'nr_packed', 'value')
    __slots__ = ('key', 'gen', 'weights', 'inputs', 'injected') + _PAYLOAD

    def __init__(self, key=None, gen=None, weights=None, inputs=None, injected=False, **payload):
        self.key, self.gen, self.injected = key, gen, injected
        self.weights = None if weights is None else _resident(weights)
        self.inputs = None if inputs is None else _resident(inputs)
        for name in self._PAYLOAD:
            setattr(self, name, payload.pop(name, None))
        if payload:
            raise TypeError('Kept: no payload named %s' % ', '.join(sorted(payload)))

    def built_from(self, key, gen, params):
        """The weights test: the same plain key, built in this weights generation, from parameters still resident."""
        return self.key == key and self.gen == gen and _still_resident(self.weights, params)

    def fed_by(self, tensors, equal_by_value=None):
        """The input ladder: the remembered objects hit; otherwise ``equal_by_value()``, when given, is asked once and
        on True these objects are remembered, so that the frames that follow hit by identity; otherwise a miss.
        Without the callable nothing is compared by value, i.e. nothing synchronises."""
        if _still_resident(self.inputs, tensors):
            return True
        if equal_by_value is not None and equal_by_value():
            self.remember(tensors)
            return True
        return False

    def remember(self, tensors):
        self.inputs = _resident(tensors)

"""The CSS network of the reference (networks/) with the output head on the device."""

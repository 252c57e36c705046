unsigned int sleep(unsigned int seconds) { (void)seconds; return 0; } /* linked in front of libc's: a burst does not cost a second */
